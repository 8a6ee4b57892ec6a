"""Inputs off the unit cube: the two relations of tests/test_gpu_domains.py, tests/test_domains_host.py and tools/domain_errors.py,
the transforms behind them, and the case table -- one small existing case per entry family that reads coordinates.

1. Power-of-two scales.  Every covariance here is a function of (x - x') / l.  ``scaled(problem, roles, k)`` multiplies dimension d
   of every coordinate array and its lengthscale by 2^k_d (exact in binary floating point), so x_d / l_d is the same double and the
   device's answer on the scaled problem is, bit for bit, its answer on the original one; gradients with respect to x_d or l_d are
   exactly 2^-k_d times the original.  What is tied to the inputs moves with them: a mean function's slope A_d by 2^-k_d, the
   radii of the local penalisation by 2^k (one k for all dimensions), Kumaraswamy's xmin / xmax and Gower's ranges by 2^k_d.
   EXPONENTS cycles over the dimensions; a model with one lengthscale takes one exponent: UNIFORM's, one after the other.
2. Offsets.  ``shifted(problem, roles, off)`` adds OFFSETS (cycled) to every coordinate array; nothing is scaled.  x + 1000 rounds
   (for plain draws of U(0, 1); see the last paragraph for the anchor's data), so the reference is the family's long-double truth ON THE SHIFTED ARRAYS, and the allowance is  existing + 2 Delta:  existing
   is what the entry's own test grants (``Family.tolerance``), Delta (``shifted_truth``) is what no double implementation that rounds
   x_d / l_d once can avoid -- the largest max-norm difference between the truth on the given inputs and the truth on inputs
   replaced by l_d fl64(x_d / l_d) (and by l_d fl64(x_d fl64(1 / l_d))), the products formed in long double.  The factor 2 covers
   the terms of second order and entries whose two sides are scaled in different kernels.  ``condition`` holds 2 Delta to ten
   times the existing tolerance, so that the allowance cannot swallow a real error; tests/test_domains_host.py asserts it.

A family states: where its problem comes from (an existing case module -- no new problems), the roles of the problem's arrays, its
long-double truth as a function of the arrays as given, the existing tolerances, how the device is driven (``device(h, p)``: every
result under a name), and per result whether part 1 holds it bit for bit (EXACT), after multiplying a gradient back by 2^k_d
(grad(axis)), or leaves it out -- with the formula that is not homogeneous.  Nothing here needs a GPU, and the library is only
imported inside ``device``.

Where the table departs from "one ARD and one non-ARD case, the smallest that crosses a 128-row tile, N <= 300":
* the sparse cases take a first offset of 250 and 31.25 instead of 1000 (their tolerance is a few 1e-13 of the scale: with 1000,
  2 Delta exceeds ten times it); every other case keeps 1000;
* the local penalisation, Gower, the ensemble, entropy search and input warping have one case each: the existing case modules hold
  no second one of N <= 300 (the ensemble's only other small case is the one on the jitter ladder, whose truth depends on the rung);
* tests/_ehvi_truth.py's cases all have N = 120, one row tile;
* the ensemble runs the first three of case t's 64 members (Delta costs two truths per member's lengthscales);
* ``NOT_COVERED`` lists the one method that takes coordinates and that no family runs (the replica group's Gower set-up), with
  the reason; the batched fits, the sparse posterior samples and the replica group run inside the dense, input-warping, sparse
  and local-penalisation families;
* the dense anchor's coordinates (and with them those of the local penalisation, Gower and entropy search) are case j's
  fl(u + 1000) - 1000, multiples of 2^-43: adding 1000 or -37.5 back is exact, so in these four families part 2 never holds a
  rounded x + off -- x / l still rounds.  The other families' data are plain U(0, 1) draws, whose shifted values do round.
"""
import collections
import functools

import numpy as np

from oracle import cpu_ref as O

import _cost_truth as CT
import _family_shapes as FS
import _kernel_families as KF
import _mean_truth as MT
import _paths_truth as PT
import _sparse_ref as SR

T = np.longdouble
LD, F64 = SR.LD, SR.F64
EPS_LD = float(np.finfo(T).eps)

EXPONENTS = (-17, 10, 0, -3, 6)          # k_d, cycled over the dimensions: ranges that differ by 10^8, far from over- and underflow
UNIFORM = (-17, 10)                      # one lengthscale, one exponent: first the one, then the other
OFFSETS = (1000.0, -37.5, 0.0, 12.0)     # cycled over the dimensions

# the roles of a problem's arrays
COORD, LENGTH, SLOPE, RADIUS = "coordinate", "lengthscale", "slope", "radius"

EXACT = "exact"
Grad = collections.namedtuple("Grad", "axis power")      # index d runs along ``axis``; the result moves by 2^(power k_d): -1 for a
#                                                          gradient with respect to x_d or l_d, +1 for one with respect to a slope A_d
Index = collections.namedtuple("Index", "of sense")      # a row index: the arg-best of result ``of`` (-1: smallest, +1: largest)
LeftOut = collections.namedtuple("LeftOut", "why")       # not homogeneous by its own formula: part 2 only


def grad(axis=-1, power=-1):
    return Grad(axis, power)


def exponents(D, uniform=None):
    """k [D]: EXPONENTS cycled, or ``uniform`` in every dimension."""
    if uniform is not None:
        return np.full(D, int(uniform))
    return np.array([EXPONENTS[d % len(EXPONENTS)] for d in range(D)])


def offsets(D, first=OFFSETS[0]):
    """off [D]: OFFSETS cycled; ``first`` replaces the list's first entry for a case whose condition asks for a smaller one."""
    return np.array([(first if d % len(OFFSETS) == 0 else OFFSETS[d % len(OFFSETS)]) for d in range(D)], dtype=float)


def _each(a, fn):
    """fn over an array, or over every array of a tuple of them (a family with several data sets)."""
    if a is None:
        return None
    if isinstance(a, tuple):
        return tuple(_each(b, fn) for b in a)
    return fn(np.asarray(a))


def _one(v):
    assert np.all(v == v.flat[0]), "one lengthscale (or a radius) takes one exponent for all dimensions"
    return v.flat[0]


def only(role, dims, D):
    """``role`` in the listed dimensions alone (the others hold something that does not move: a warped coordinate in [0, 1])."""
    mask = np.zeros(D, dtype=bool)
    mask[list(dims)] = True
    return (role, tuple(mask))


def _masked(role, v, neutral):
    """(role, v) with v's entries outside a masked role's dimensions replaced by ``neutral``."""
    if isinstance(role, tuple):
        return role[0], np.where(np.array(role[1]), v, neutral)
    return role, v


def scaled(p, roles, k):
    """The problem with dimension d of every coordinate and lengthscale multiplied by 2^k_d -- and what is tied to them."""
    s_all = 2.0 ** np.asarray(k, dtype=float)
    q = dict(p)
    for key, role in roles.items():
        role, s = _masked(role, s_all, 1.0)
        if role == COORD:
            q[key] = _each(p[key], lambda a: a * s)
        elif role == LENGTH:
            q[key] = _each(p[key], lambda a: a * (s if a.shape[-1] == s.size else _one(s)))
        elif role == SLOPE:                                     # A [D, P]:  A_d x_d is what must not move
            q[key] = _each(p[key], lambda a: a / s[:, None])
        elif role == RADIUS:
            q[key] = _each(p[key], lambda a: a * _one(s))
        else:
            raise KeyError(role)
    return q


def shifted(p, roles, off):
    """The problem with ``off`` added to every coordinate array; nothing else moves."""
    off_all = np.asarray(off, dtype=float)
    q = dict(p)
    for key, role in roles.items():
        role, off = _masked(role, off_all, 0.0)
        if role == COORD:
            q[key] = _each(p[key], lambda a: a + off)
    return q


def rounded(p, roles, ls, how):
    """The problem with every coordinate replaced by l_d fl64(x_d / l_d) (``how`` = "div") or l_d fl64(x_d fl64(1 / l_d)) ("mul"),
    the outer product formed -- and kept -- in long double.  ``ls`` [D] is the lengthscale of every dimension."""
    ls = np.asarray(ls, dtype=np.float64)
    q = dict(p)
    for key, role in roles.items():
        role, on = _masked(role, np.ones(ls.size, dtype=bool), False)

        def fn(a):
            a = np.asarray(a, dtype=np.float64)
            u = a / ls if how == "div" else a * (1.0 / ls)
            return np.where(on, u.astype(T) * ls.astype(T), a.astype(T))

        if role == COORD:
            q[key] = _each(p[key], fn)
    return q


def unscale(kind, a, k):
    """A result of the scaled problem brought back: a gradient times 2^(-power k_d) along its axis (exact); everything else as it
    is."""
    a = np.asarray(a)
    if not isinstance(kind, Grad):
        return a
    s = 2.0 ** (-kind.power * np.asarray(k, dtype=float))
    n = a.shape[kind.axis]
    if n != s.size:                                             # one lengthscale: one exponent
        assert n == 1
        return a * _one(s)
    shape = [1] * a.ndim
    shape[kind.axis] = n
    return a * s.reshape(shape)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b) and a.tobytes() == b.tobytes()


def part1_failures(results, base, moved, k):
    """The names of the results whose bits the scaling moved: ``base`` and ``moved`` are a family's outputs (device or truth) on the
    original and on the scaled problem.  -0.0 against 0.0 counts as moved."""
    bad = []
    for name, kind in results.items():
        if isinstance(kind, LeftOut):
            continue
        a, b = np.asarray(base[name]), unscale(kind, moved[name], k)
        if not same_bits(np.asarray(a, dtype=b.dtype), b):
            diff = np.asarray(a, dtype=T) - np.asarray(b, dtype=T)
            bad.append("%s (largest difference %.3e)" % (name, float(np.max(np.abs(diff))) if a.shape == b.shape else np.nan))
    return bad


def part1_truth_gap(results, base, moved, k):
    """Relation 1 on the long-double truths: the largest |moved back - base| over the largest |base| per result, in units of the
    long-double eps (tests/test_domains_host.py holds it to a few)."""
    out = {}
    for name, kind in results.items():
        if isinstance(kind, (LeftOut, Index)):
            continue
        a, b = np.asarray(base[name], dtype=T), np.asarray(unscale(kind, np.asarray(moved[name], dtype=T), k), dtype=T)
        out[name] = float(np.max(np.abs(a - b)) / max(np.max(np.abs(a)), T(1e-300))) / EPS_LD
    return out


def maxnorm(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=T) - np.asarray(b, dtype=T))))


# ---- long-double pieces shared by the families ---------------------------------------------------------------------------------------
def _ld(a):
    return None if a is None else np.asarray(a, dtype=T)


class _GP(MT.MeanGP):
    """tests/_mean_truth.py's exact GP in long double on arrays as given (long-double coordinates included), with the LML's
    gradient with respect to the training inputs beside the hyper-gradients."""

    def __init__(self, fam, ard, variance, ls, noise, X, Y, A=None, b=None):
        MT.MeanGP.__init__(self, fam, ard, variance, np.asarray(ls, dtype=float), noise, _ld(X), np.asarray(Y, dtype=T), A, b, LD)

    def all_gradients(self):
        """(dvariance, dlengthscale, dnoise, dL/dX [N, D], dA, db)."""
        N, P = self.R.shape
        Ki = LD.solve(self.L, LD.solve(self.L, np.eye(N, dtype=T), 0), 1)
        dL_dK = (self.alpha @ self.alpha.T - P * Ki) / 2
        dvar, dls = self.kern.update_gradients_full(dL_dK, self.X)
        return dvar, dls, np.trace(dL_dK), self.kern.gradients_X(dL_dK, self.X), self.X.T @ self.alpha, self.alpha.sum(0)

    def fmin(self):
        return self.train_mean()[:, 0].min()


class _pinned(object):
    """The float64 yardsticks of the tolerances (the pinned oracle, the float64 restatements) with every BLAS / OpenMP pool held
    to one thread: a threaded BLAS sums in an order that depends on the thread count, and a tolerance that is a multiple of the
    yardstick's own rounding error would move with it (the sparse case S2's dvariance, a cancelling sum of three terms of 1.5e4
    each: 3.0e-11 with eight threads, 8.1e-11 with one).  One thread is one order."""

    def __enter__(self):
        self.keep = O.limit_blas_threads(1)[0]
        return self

    def __exit__(self, *exc):
        if self.keep is not None:
            self.keep.restore_original_limits()
        return False


RULES = (("EI", 0.01), ("LCB", 2.0), ("MPI", 0.01))


def _acq_id(name):
    from gaussian_process_optimization_amd import _lib
    return {"EI": _lib.GP_ACQ_EI, "LCB": _lib.GP_ACQ_LCB, "MPI": _lib.GP_ACQ_MPI}[name]


def _kernel_id(fam):
    return FS.KERNEL_ID[fam]


def _scores(name, mu, var1, dm, dv, fmin):
    """The oracle's rule on a long-double posterior (tests/_mean_truth.scores: the rule itself runs in double)."""
    v, g = MT.scores(name, np.asarray(mu, dtype=float), np.asarray(var1, dtype=float), np.asarray(dm, dtype=float),
                     np.asarray(dv, dtype=float), float(fmin))
    return v[:, None], g


def _rel(t, tol=1e-6, floor=0.0):
    """tol of the largest reference entry: the convention of tests/test_gpu_kernel_families.py's _err."""
    return tol * max(float(np.max(np.abs(np.asarray(t, dtype=T)))), floor)


class Family(object):
    """One row of the table."""
    name = source = None
    ard = True
    first_offset = OFFSETS[0]
    offset_note = ""
    roles = {}
    results = {}
    methods = ()              # the Handle methods (and pack methods) whose coordinates this family moves

    def problem(self):
        raise NotImplementedError

    def D(self):
        return int(np.asarray(self.lengthscales(self.problem())[0]).size)

    def lengthscales(self, p):
        """The per-dimension lengthscales [D] a coordinate is divided by: one vector per model of the family."""
        ls = np.asarray(p["ls"], dtype=float).reshape(-1)
        D = np.asarray(p["X"][0] if isinstance(p["X"], tuple) else p["X"]).shape[1]
        return [ls if ls.size == D else np.full(D, ls[0])]

    uniform = None            # one exponent for all dimensions; None: where the model has one lengthscale

    def exponent_sets(self):
        D = self.D()
        one = (not self.ard) if self.uniform is None else self.uniform
        return [exponents(D, u) for u in UNIFORM] if one else [exponents(D)]

    def offset(self):
        return offsets(self.D(), self.first_offset)

    def result_exponents(self, k):
        """The exponents a result's gradients are multiplied back by: those of the problem."""
        return k

    def truth(self, p):
        raise NotImplementedError

    def tolerance(self, p, t):
        raise NotImplementedError

    def device(self, h, p):
        raise NotImplementedError


# ---- 1. the dense anchor: tests/_family_shapes.py case j's problem -------------------------------------------------------------------------
class Dense(Family):
    """fit, hyper- and input gradients, the table entries on 130 candidates (two candidate tiles), the small-M route on 5, the
    one-location calls on 3 (fused, one pass) and 8 rows (fused, wide), and the R = 3 members of the batched fit.  Truth: the
    long-double GP of tests/_mean_truth.py without a mean; tolerances: tests/test_gpu_family_shapes.py's."""
    source = "_family_shapes case j (N = 300, D = 3, M = 130), without its offset"
    roles = {"X": COORD, "Xs": COORD, "ls": LENGTH, "ls_members": LENGTH}
    methods = ("set_data", "set_params", "set_candidates", "cross_kernel_matrix", "predict_rows", "mean_grad_rows", "acq_rows",
               "fit_grad_batch", "fit_grad_warp_batch")
    results = collections.OrderedDict(
        [(n, EXACT) for n in ("K", "Kx", "lml", "logdet", "jitter", "alpha", "fmin", "dvariance", "dnoise")]
        + [("dlengthscale", grad(0)), ("dL_dX", grad(1))]
        + [(n, EXACT) for n in ("mean", "var", "var0")] + [("dmdx", grad(1)), ("dvdx", grad(1))]
        + [(n, EXACT) for n in ("cov",)]
        + sum([[(r, EXACT), ("d" + r, grad(1)), (r + " argbest", Index(r, -1))] for r, _ in RULES], [])
        + [("small_m mean", EXACT), ("small_m var", EXACT), ("small_m dmdx", grad(1)), ("small_m dvdx", grad(1)),
           ("small_m EI", EXACT), ("small_m dEI", grad(1))]
        + sum([[("rows%d mean" % k, EXACT), ("rows%d var" % k, EXACT), ("rows%d dmdx" % k, grad(1)), ("rows%d dvdx" % k, grad(1)),
                ("rows%d EI" % k, EXACT), ("rows%d dEI" % k, grad(1)), ("rows%d dmdx alone" % k, grad(1))] for k in (3, 8)], [])
        + [("members lml", EXACT), ("members logdet", EXACT), ("members dvariance", EXACT), ("members dlengthscale", grad(1)),
           ("members dnoise", EXACT)]
        + [("warp logdet", EXACT), ("warp log_jacobian", EXACT), ("warp dvariance", EXACT), ("warp dlengthscale", grad(1))])
    WARPS = ("A", "B")        # tests/_warped_ref.PARAMS: three tanh terms each, for members 0 and 1 of the batched output-warped fit

    def _warps(self):
        import _warped_ref as WR
        return np.array([WR.PARAMS[w][0] for w in self.WARPS]), np.array([WR.PARAMS[w][1] for w in self.WARPS])

    def __init__(self, fam, ard):
        self.fam, self.ard = fam, ard
        self.name = "dense anchor, %s %s" % (fam, "ARD" if ard else "one lengthscale")

    @functools.lru_cache(maxsize=None)
    def problem(self):
        c = FS.CASES["j"]
        X, Y, Xs, ls = FS.problem("j")
        X, Xs = X - c.off, Xs - c.off            # (exact: the case adds 1000 to numbers in [0, 1], and the difference is Sterbenz's)
        Xs = Xs.copy()
        Xs[0] = X[FS.coincident_row(c)]
        ls = np.array(ls) if self.ard else np.array([0.35 * np.sqrt(c.D)])       # the iso rule of tests/_family_shapes.problem
        return dict(X=X, Y=np.array(Y), Xs=Xs, ls=ls, ls_members=np.array([ls, ls * 2.2, ls * 0.6]),
                    var_members=np.array([FS.VAR, 0.4, 2.5]), noise_members=np.array([FS.NOISE, 3e-2, 2e-3]))

    def truth(self, p):
        gp = _GP(self.fam, self.ard, FS.VAR, p["ls"], FS.NOISE, p["X"], p["Y"])
        X, Xs = _ld(p["X"]), _ld(p["Xs"])
        t = collections.OrderedDict()
        t["K"], t["Kx"] = gp.Kf, gp.kern.K(X, Xs)
        t["lml"], t["logdet"], t["jitter"], t["alpha"], t["fmin"] = gp.lml, gp.logdet, T(0), gp.alpha, gp.fmin()
        t["dvariance"], t["dlengthscale"], t["dnoise"], t["dL_dX"], _, _ = gp.all_gradients()
        mu, v0, v1, dm, dv = gp.at(Xs)
        t["mean"], t["var"], t["var0"], t["dmdx"], t["dvdx"] = mu, v1[:, None], v0[:, None], dm, dv
        kx = gp.kern.K(Xs[:9], X)
        w = LD.solve(gp.L, kx.T, 0)
        t["cov"] = gp.kern.K(Xs[:9]) - w.T @ w + gp.noise * np.eye(9, dtype=T)
        for r, _ in RULES:
            t[r], t["d" + r] = _scores(r, mu[:, 0], v1, dm[:, :, 0], dv, t["fmin"])
            t[r + " argbest"] = np.array(int(np.argmin(t[r][:, 0])))
        t["small_m mean"], t["small_m var"], t["small_m dmdx"], t["small_m dvdx"] = mu[:5], v1[:5, None], dm[:5], dv[:5]
        t["small_m EI"], t["small_m dEI"] = t["EI"][:5], t["dEI"][:5]
        for k in (3, 8):
            n = "rows%d " % k
            t[n + "mean"], t[n + "var"], t[n + "dmdx"], t[n + "dvdx"] = mu[:k], v1[:k, None], dm[:k], dv[:k]
            t[n + "EI"], t[n + "dEI"], t[n + "dmdx alone"] = t["EI"][:k], t["dEI"][:k], dm[:k]
        rec = []
        for m in range(3):
            g = gp if m == 0 else _GP(self.fam, self.ard, p["var_members"][m], p["ls_members"][m], p["noise_members"][m], p["X"], p["Y"])
            dvar, dls, dn = g.all_gradients()[:3] if m else (t["dvariance"], t["dlengthscale"], t["dnoise"])
            rec.append((g.lml, g.logdet, dvar, dls, dn))
        for i, n in enumerate(("lml", "logdet", "dvariance", "dlengthscale", "dnoise")):
            t["members " + n] = np.array([r[i] for r in rec], dtype=T)
        import _warped_ref as WR
        psis, ds = self._warps()
        rec = []
        for m in range(2):                       # the GP of member m's parameters on the tanh-warped targets, and the log-Jacobian
            Yw = WR.f(p["Y"], psis[m], ds[m], T)
            g = _GP(self.fam, self.ard, p["var_members"][m], p["ls_members"][m], p["noise_members"][m], p["X"], Yw)
            dvar, dls = g.all_gradients()[:2]
            rec.append((g.logdet, np.log(WR.fgrad_y(p["Y"], psis[m], ds[m], T)).sum(), dvar, dls))
        for i, n in enumerate(("logdet", "log_jacobian", "dvariance", "dlengthscale")):
            t["warp " + n] = np.array([r[i] for r in rec], dtype=T)
        return t

    def tolerance(self, p, t):
        """tests/test_gpu_family_shapes.py: K 1e-13 of the variance plus the derived rounding of x / l (_family_shapes.k_tolerance),
        LML 1e-8, log det 1e-10, the variance with noise 1e-6 of itself, everything else 1e-6 of the largest reference entry, the
        hyper-gradients on _grad_err's scales."""
        D = p["X"].shape[1]
        ls = self.lengthscales(p)[0]
        big = max(float(np.max(np.abs(p["X"] / ls))), float(np.max(np.abs(p["Xs"] / ls))))
        ktol = FS.VAR * (1e-13 + 2.0 * np.sqrt(D) * 2.0 ** -53 * big)
        tol = {n: _rel(v) for n, v in t.items() if not isinstance(self.results[n], Index)}
        tol.update(K=ktol, Kx=ktol, lml=1e-8 * abs(float(t["lml"])), logdet=1e-10 * abs(float(t["logdet"])), jitter=0.0,
                   fmin=1e-6 * max(1.0, abs(float(t["fmin"]))), var0=1e-6 * FS.VAR)
        for n in ("var", "small_m var", "rows3 var", "rows8 var"):
            tol[n] = 1e-6 * np.asarray(t[n], dtype=float)
        gs = max(abs(float(t["dvariance"])), float(np.max(np.abs(t["dlengthscale"]))), 1.0)
        tol.update(dvariance=1e-6 * gs, dlengthscale=1e-6 * gs, dnoise=1e-6 * max(abs(float(t["dnoise"])), 1.0))
        tol["members lml"] = 1e-8 * np.abs(np.asarray(t["members lml"], dtype=float))
        tol["members logdet"] = 1e-10 * np.abs(np.asarray(t["members logdet"], dtype=float))
        ms = np.maximum(np.maximum(np.abs(t["members dvariance"]), np.abs(t["members dlengthscale"]).max(1)), 1.0).astype(float)
        tol["members dvariance"], tol["members dlengthscale"] = 1e-6 * ms, 1e-6 * ms[:, None] * np.ones_like(t["members dlengthscale"], dtype=float)
        tol["members dnoise"] = 1e-6 * np.maximum(np.abs(t["members dnoise"]), 1.0).astype(float)
        tol["warp logdet"] = 1e-10 * np.abs(np.asarray(t["warp logdet"], dtype=float))
        tol["warp log_jacobian"] = 1e-10 * np.maximum(np.abs(np.asarray(t["warp log_jacobian"], dtype=float)), 1.0)     # a sum of N logarithms
        ws = np.maximum(np.maximum(np.abs(t["warp dvariance"]), np.abs(t["warp dlengthscale"]).max(1)), 1.0).astype(float)
        tol["warp dvariance"], tol["warp dlengthscale"] = 1e-6 * ws, 1e-6 * ws[:, None] * np.ones_like(t["warp dlengthscale"], dtype=float)
        return tol

    def device(self, h, p):
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id(self.fam), int(self.ard), FS.VAR, p["ls"], FS.NOISE)
        d = collections.OrderedDict()
        d["K"], d["Kx"] = h.kernel_matrix(), h.cross_kernel_matrix(p["Xs"])
        nls = p["ls"].size
        (lml, logdet, jit), (dv, dl, dn) = h.fit_grad(nls)
        d["lml"], d["logdet"], d["jitter"], d["alpha"] = np.array(lml), np.array(logdet), np.array(jit), h.alpha()
        fmin = h.fmin()
        d["fmin"], d["dvariance"], d["dlengthscale"], d["dnoise"], d["dL_dX"] = np.array(fmin), np.array(dv), dl, np.array(dn), h.lml_grad_x()
        h.set_candidates(p["Xs"])
        d["mean"], d["var"] = h.predict(True)
        d["var0"] = h.predict(False)[1]
        d["dmdx"], d["dvdx"] = h.predict_grad()
        for r, par in RULES:
            d[r], d["d" + r] = h.acq_grad(_acq_id(r), par, fmin)
            d[r + " argbest"] = np.array(h.acq_argbest(_acq_id(r), par, fmin, -1)[0])
        h.set_candidates(p["Xs"][:9])
        d["cov"] = h.predict_full_cov(True)[1]
        h.set_candidates(p["Xs"][:5])
        d["small_m mean"], d["small_m var"] = h.predict(True)
        d["small_m dmdx"], d["small_m dvdx"] = h.predict_grad()
        d["small_m EI"], d["small_m dEI"] = h.acq_grad(_acq_id("EI"), 0.01, fmin)
        for k in (3, 8):
            n, x = "rows%d " % k, np.ascontiguousarray(p["Xs"][:k])
            d[n + "mean"], d[n + "var"], d[n + "dmdx"], d[n + "dvdx"] = h.predict_rows(x, True, grad=True)
            d[n + "EI"], d[n + "dEI"] = h.acq_rows(x, _acq_id("EI"), 0.01, fmin, grad=True)
            d[n + "dmdx alone"] = h.mean_grad_rows(x)
        (lml, logdet, jit), (dv, dl, dn), status = h.fit_grad_batch(p["var_members"], p["ls_members"], p["noise_members"])
        assert not status.any() and not jit.any()
        d["members lml"], d["members logdet"], d["members dvariance"], d["members dlengthscale"], d["members dnoise"] = lml, logdet, dv, dl, dn
        psis, ds = self._warps()
        (_, logdet, jit), (dv, dl, _), lj, _, status = h.fit_grad_warp_batch(psis, ds, p["var_members"][:2], p["ls_members"][:2],
                                                                            p["noise_members"][:2])
        assert not status.any() and not jit.any()
        d["warp logdet"], d["warp log_jacobian"], d["warp dvariance"], d["warp dlengthscale"] = logdet, lj, dv, dl
        return d

    def lengthscales(self, p):
        D = p["X"].shape[1]
        return [np.broadcast_to(l, (D,)) if l.size == 1 else l for l in np.asarray(p["ls_members"], dtype=float)]


# ---- 2. the local penalisation over the dense anchor's model ----------------------------------------------------------------------------
LP_GRADIENT = ("d/dx [-log EI(x) - sum_b log Phi(z_b)], z_b = (|x - Xb_b| - r_b) / s_b:  the penaliser's term is "
               "phi(z_b) / (Phi(z_b) s_b |x - Xb_b|), summed over the batch and broadcast over the dimensions (LP.py:91-103 as the "
               "reference has it): under x -> 2^k x it moves by 2^-2k, the base term dEI / EI by 2^-k")


def _lp_truth(v, g, x, Xb, r0, s0):
    """oracle.cpu_ref.lp_penalized_acquisition / lp_d_acquisition (transform "none") with the distances and log Phi in long double
    (tests/_feas_truth.log_ndtr, mills)."""
    import _feas_truth as FT
    x, Xb = _ld(x), _ld(Xb)
    fval = np.asarray(-v[:, 0], dtype=T)
    nm = np.sqrt(((x[:, None, :] - Xb[None, :, :]) ** 2).sum(-1))
    z = (nm - _ld(r0)) / _ld(s0)
    val = -np.log(fval + T(1e-50)) - FT.log_ndtr(z).sum(-1)
    d = FT.mills(z) / (_ld(s0) * nm)
    return val, np.asarray(g, dtype=T) / fval[:, None] - d.sum(1)[:, None]


class LocalPenalisation(Family):
    """gp_acq_lp / gp_acq_lp_grad / gp_acq_lp_argbest and the one-location call with a penaliser, EI with transform "none" and a
    batch of two, on the dense anchor's model; the radii r_x0, s_x0 are distances in x, so the scale is one for all dimensions."""
    name = "local penalisation"
    source = "_family_shapes case j; batch and radii as tests/test_gpu_kernel_families.py draws them (rows 20, 41 + 0.013, L = 3.1)"
    uniform = True
    fam = "Mat52"
    roles = {"X": COORD, "Xs": COORD, "Xb": COORD, "ls": LENGTH, "r0": RADIUS, "s0": RADIUS}
    methods = ("acq_lp", "acq_lp_grad", "acq_lp_argbest", "acq_rows", "Group.set_data", "Group.set_params", "Group.set_candidates",
               "Group.acq_lp_argbest")
    results = collections.OrderedDict([("lp", EXACT), ("lp (gradient call)", EXACT), ("dlp", LeftOut(LP_GRADIENT)),
                                       ("lp argbest", Index("lp", -1)), ("rows6 lp", EXACT), ("rows6 dlp", LeftOut(LP_GRADIENT)),
                                       ("EI", EXACT), ("group lml", EXACT), ("group fmin", EXACT), ("group EI argbest", Index("EI", -1)),
                                       ("group EI best", EXACT), ("group lp argbest", Index("lp", -1)), ("group lp best", EXACT)])

    @functools.lru_cache(maxsize=None)
    def problem(self):
        p = dict(FAMILIES["dense anchor, Mat52 ARD"].problem())
        Xb = np.array(p["Xs"][[20, 41]] + 0.013)
        gm = O.OracleGPModel(O.OracleGP(p["X"], p["Y"], KF.make(self.fam, 3, FS.VAR, p["ls"], True, direct=True), FS.NOISE))
        r0, s0 = O.lp_hammer_precompute(gm, Xb, 3.1, float(p["Y"].min()))
        return dict(X=p["X"], Y=p["Y"], Xs=p["Xs"], ls=p["ls"], Xb=Xb, r0=np.array(r0), s0=np.array(s0))

    def truth(self, p):
        gp = _GP(self.fam, True, FS.VAR, p["ls"], FS.NOISE, p["X"], p["Y"])
        mu, v0, v1, dm, dv = gp.at(_ld(p["Xs"]))
        v, g = _scores("EI", mu[:, 0], v1, dm[:, :, 0], dv, gp.fmin())
        lp, dlp = _lp_truth(v, g, p["Xs"], p["Xb"], p["r0"], p["s0"])
        t = collections.OrderedDict([("lp", lp), ("lp (gradient call)", lp), ("dlp", dlp)])
        t["lp argbest"] = np.array(int(np.argmin(lp)))
        t["rows6 lp"], t["rows6 dlp"] = lp[:6], dlp[:6]
        # the replica group: the model on two replicas of one device, the table split over them, the winners merged
        t["EI"], t["group lml"], t["group fmin"] = v, gp.lml, gp.fmin()
        t["group EI argbest"], t["group EI best"] = np.array(int(np.argmin(v[:, 0]))), np.min(v[:, 0])
        t["group lp argbest"], t["group lp best"] = t["lp argbest"], np.min(lp)
        return t

    def tolerance(self, p, t):
        """tests/test_gpu_kernel_families.py: 1e-6 of the largest reference entry (a winner's value: of the table's largest), the
        LML 1e-8, fmin 1e-6 max(1, |fmin|)."""
        tol = {n: _rel(v) for n, v in t.items() if not isinstance(self.results[n], Index)}
        tol.update({"group lml": 1e-8 * abs(float(t["group lml"])), "group fmin": 1e-6 * max(1.0, abs(float(t["group fmin"]))),
                    "group EI best": tol["EI"], "group lp best": tol["lp"]})
        return tol

    def device(self, h, p):
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id(self.fam), 1, FS.VAR, p["ls"], FS.NOISE)
        h.fit()
        fmin, ei = h.fmin(), _acq_id("EI")
        h.set_candidates(p["Xs"])
        d = collections.OrderedDict()
        d["lp"] = h.acq_lp(ei, 0.01, fmin, 0, p["Xb"], p["r0"], p["s0"])
        d["lp (gradient call)"], d["dlp"] = h.acq_lp_grad(ei, 0.01, fmin, 0, p["Xb"], p["r0"], p["s0"])
        d["lp argbest"] = np.array(h.acq_lp_argbest(ei, 0.01, fmin, 0, -1, p["Xb"], p["r0"], p["s0"])[0])
        v, dv = h.acq_rows(np.ascontiguousarray(p["Xs"][:6]), ei, 0.01, fmin, grad=True, lp=(0, p["Xb"], p["r0"], p["s0"]))
        d["rows6 lp"], d["rows6 dlp"] = np.ravel(v), dv
        d["EI"] = h.acq(ei, 0.01, fmin)
        from gaussian_process_optimization_amd import _lib
        g = _lib.Group([0, 0])
        try:
            g.set_option("emulate_fp64", 0)
            g.set_data(p["X"], p["Y"])
            g.set_params(_kernel_id(self.fam), 1, FS.VAR, p["ls"], FS.NOISE)
            d["group lml"] = np.array(g.fit()[0])
            gf = g.fmin()
            d["group fmin"] = np.array(gf)
            g.set_candidates(p["Xs"])
            i, val = g.acq_argbest(ei, 0.01, gf, -1)
            d["group EI argbest"], d["group EI best"] = np.array(i), np.array(val)
            i, val = g.acq_lp_argbest(ei, 0.01, gf, 0, -1, p["Xb"], p["r0"], p["s0"])
            d["group lp argbest"], d["group lp best"] = np.array(i), np.array(val)
        finally:
            g.close()
        return d


# ---- 3. Gower's product kernel ------------------------------------------------------------------------------------------------------------
class Gower(Family):
    """gp_set_gower: k(x, x') = prod_d k(|x_d - x'_d| / range_d) over the continuous dimensions times k(x_d != x'_d) over the
    discrete ones (stationary.py:116-135 of the fork, oracle.cpu_ref.Stationary.K).  Two continuous dimensions (ranges 0.7 and 1.9:
    x / range rounds) and one discrete (levels 0 .. 3, the third: its exponent and its offset are 0); the ranges follow the scale.  Truth: that product in long
    double, then the exact GP's algebra."""
    name = "Gower"
    source = "_family_shapes case j with its third coordinate replaced by levels, as tests/test_gpu_mean_function.py does"
    fam = "Mat52"
    roles = {"X": COORD, "Xs": COORD, "ls": LENGTH, "ranges": LENGTH}
    methods = ("set_gower",)
    results = collections.OrderedDict((n, EXACT) for n in ("K", "Kx", "lml", "logdet", "alpha", "mean"))
    DISC = np.array([0, 0, 1])

    @functools.lru_cache(maxsize=None)
    def problem(self):
        p = FAMILIES["dense anchor, Mat52 ARD"].problem()
        rng = np.random.default_rng(77)
        X, Xs = p["X"].copy(), p["Xs"].copy()
        X[:, 2], Xs[:, 2] = rng.integers(0, 4, X.shape[0]), rng.integers(0, 4, Xs.shape[0])
        Xs[0] = X[5]
        return dict(X=X, Y=p["Y"], Xs=Xs, ls=p["ls"], ranges=np.array([0.7, 1.9, 1.0]))

    def lengthscales(self, p):
        return [np.asarray(p["ranges"], dtype=float)]

    def _K(self, A, B, ranges):
        A, B = _ld(A), _ld(B)
        K = None
        for d in range(A.shape[1]):
            if self.DISC[d]:
                r = (A[:, None, d] != B[None, :, d]).astype(T)
            else:
                r = np.abs(A[:, None, d] - B[None, :, d]) / T(ranges[d])
            k = SR.k_of_r(self.fam, T(FS.VAR), r)
            K = k if K is None else K * k
        return K

    def truth(self, p):
        X, Y = p["X"], np.asarray(p["Y"], dtype=T)
        N, P = Y.shape
        K = self._K(X, X, p["ranges"])
        Ky = K + (T(FS.NOISE) + T(MT.CONST_DIAG)) * np.eye(N, dtype=T)
        L = LD.chol(Ky)[0]
        alpha = LD.solve(L, LD.solve(L, Y, 0), 1)
        logdet = 2 * np.sum(np.log(np.diag(L)))
        Kx = self._K(X, p["Xs"], p["ranges"])
        return collections.OrderedDict([("K", K), ("Kx", Kx), ("lml", -(N * P * np.log(2 * T(np.pi)) + P * logdet + np.sum(alpha * Y)) / 2),
                                        ("logdet", logdet), ("alpha", alpha), ("mean", Kx.T @ alpha)])

    def tolerance(self, p, t):
        """K as the dense anchor's (1e-13 of the largest entry, variance^D, plus the rounding of x / range), the rest as
        tests/test_gpu_kernel_families.py."""
        big = max(float(np.max(np.abs(p["X"] / p["ranges"]))), float(np.max(np.abs(p["Xs"] / p["ranges"]))))
        ktol = FS.VAR ** 3 * (1e-13 + 2.0 * np.sqrt(3) * 2.0 ** -53 * big)
        return dict(K=ktol, Kx=ktol, lml=1e-8 * abs(float(t["lml"])), logdet=1e-10 * abs(float(t["logdet"])), alpha=_rel(t["alpha"]),
                    mean=_rel(t["mean"]))

    def device(self, h, p):
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id(self.fam), 1, FS.VAR, p["ls"], FS.NOISE)
        h.set_gower(self.DISC, p["ranges"])
        try:
            d = collections.OrderedDict([("K", h.kernel_matrix()), ("Kx", h.cross_kernel_matrix(p["Xs"]))])
            lml, logdet, jit = h.fit()
            assert jit == 0.0
            d["lml"], d["logdet"], d["alpha"] = np.array(lml), np.array(logdet), h.alpha()
            h.set_candidates(p["Xs"])
            d["mean"] = h.predict(True)[0]
        finally:
            h.set_gower()
        return d


# ---- 4. the mean function ------------------------------------------------------------------------------------------------------------------
class MeanFunction(Family):
    """gp_mean_set, then fit, hyper-gradients, gp_mean_grad, a table of 130, and (one output) the one-location calls and the scores.
    Truth: tests/_mean_truth.MeanGP; tolerance: tests/test_gpu_mean_function.py's max(64 e64, 1e-13 max(1, Npad / 384) scale), e64
    the pinned float64 oracle's own error against the same truth on the same arrays."""
    roles = {"X": COORD, "Xs": COORD, "ls": LENGTH, "A": SLOPE}
    methods = ("mean_set",)

    def __init__(self, cid):
        c = self.case = MT.CASES[cid]
        self.ard, self.fam = c.ard, c.fam
        self.name = "mean function, case %s" % cid
        self.source = "_mean_truth case %s (N = %d, D = %d, P = %d, %s), table of 130" % (cid, c.N, c.D, c.P, c.fam)
        r = [(n, EXACT) for n in ("lml", "logdet", "alpha", "dvariance", "dnoise", "db", "mean", "var", "var0")]
        r += [("dlengthscale", grad(0)), ("dA", grad(0, +1)), ("dmdx", grad(1)), ("dmdx alone", grad(1)), ("dvdx", grad(1))]
        if c.P == 1:
            r += [("fmin", EXACT)]
            r += sum([[(n, EXACT), ("d" + n, grad(1))] for n, _ in RULES], [])
            for k in (3, 7):
                r += [("rows%d mean" % k, EXACT), ("rows%d var" % k, EXACT), ("rows%d dmdx" % k, grad(1)), ("rows%d dvdx" % k, grad(1)),
                      ("rows%d EI" % k, EXACT), ("rows%d dEI" % k, grad(1))]
        self.results = collections.OrderedDict(r)

    @functools.lru_cache(maxsize=None)
    def problem(self):
        cid = self.case.id
        p = MT.problem(cid)
        return dict(X=p.X, Y=p.Y, Xs=MT.table(cid, 130), ls=p.ls, A=p.A, b=p.b)

    def _record(self, fit, at, train_min):
        c = self.case
        lml, logdet, alpha, dvar, dls, dn, dA, db = fit
        mu, v0, v1, dm, dv = at
        t = collections.OrderedDict(lml=lml, logdet=logdet, alpha=alpha, dvariance=dvar, dnoise=dn, db=db, mean=mu, var=v1[:, None],
                                    var0=v0[:, None], dlengthscale=dls, dA=dA, dmdx=dm)
        t["dmdx alone"], t["dvdx"] = dm, dv
        if c.P == 1:
            t["fmin"] = train_min
            for n, _ in RULES:
                t[n], t["d" + n] = _scores(n, mu[:, 0], v1, dm[:, :, 0], dv, train_min)
            for k in (3, 7):
                m = "rows%d " % k
                t[m + "mean"], t[m + "var"], t[m + "dmdx"], t[m + "dvdx"] = mu[:k], v1[:k, None], dm[:k], dv[:k]
                t[m + "EI"], t[m + "dEI"] = t["EI"][:k], t["dEI"][:k]
        return t

    def truth(self, p):
        gp = _GP(self.fam, self.ard, MT.VAR, p["ls"], MT.NOISE, p["X"], p["Y"], p["A"], p["b"])
        dvar, dls, dn, _, dA, db = gp.all_gradients()
        return self._record((gp.lml, gp.logdet, gp.alpha, dvar, dls, dn, dA, db), gp.at(_ld(p["Xs"])), gp.train_mean()[:, 0].min())

    def oracle64(self, p):
        """tests/_mean_truth.oracle64 on the arrays as given: the pinned oracle on the targets Y - m(X), m(x*) and A on the way out."""
        c = self.case
        X, x = np.asarray(p["X"], dtype=float), np.asarray(p["Xs"], dtype=float)
        gp = O.OracleGP(X, p["Y"] - MT.mean_of(p["A"], p["b"], X, np.float64), KF.make(c.fam, c.D, MT.VAR, p["ls"], c.ard, direct=True),
                        MT.NOISE)
        post = gp.posterior
        assert post["jitter"] == 0.0
        dvar, dls, dn = gp.gradients()
        mu, v0 = gp.predict_noiseless(x)
        dm, dv = gp.predictive_gradients(x)
        mu = mu + MT.mean_of(p["A"], p["b"], x, np.float64)
        if p["A"] is not None:
            dm = dm + p["A"][None, :, :]
        train = gp.predict_noiseless(X)[0] + MT.mean_of(p["A"], p["b"], X, np.float64)
        fit = (post["lml"], post["logdet"], post["alpha"], float(dvar), np.atleast_1d(np.asarray(dls, dtype=float)), float(dn),
               X.T @ post["alpha"], post["alpha"].sum(0))
        return self._record(fit, (mu, v0[:, 0], v0[:, 0] + MT.NOISE, dm, dv), train[:, 0].min())

    def tolerance(self, p, t):
        with _pinned():
            o = self.oracle64(p)
        tol = {}
        for n, v in t.items():
            e64, scale = MT.e64_of(o[n], v)
            tol[n] = max(MT.MULT * e64, MT.floor_n(self.case.N) * scale)
        return tol

    def device(self, h, p):
        c = self.case
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id(c.fam), int(c.ard), MT.VAR, p["ls"], MT.NOISE)
        h.mean_set(p["A"], p["b"])
        try:
            d = collections.OrderedDict()
            (lml, logdet, jit), (dv, dl, dn) = h.fit_grad(p["ls"].size)
            assert jit == 0.0
            d["lml"], d["logdet"], d["alpha"], d["dvariance"], d["dnoise"] = np.array(lml), np.array(logdet), h.alpha(), np.array(dv), np.array(dn)
            d["dlengthscale"] = dl
            d["dA"], d["db"] = h.mean_grad()
            h.set_candidates(p["Xs"])
            d["mean"], d["var"] = h.predict(True)
            d["var0"] = h.predict(False)[1]
            d["dmdx"], d["dvdx"] = h.predict_grad()
            d["dmdx alone"] = h.predict_grad(mean_only=True)
            if c.P == 1:
                fmin = h.fmin()
                d["fmin"] = np.array(fmin)
                for n, par in RULES:
                    d[n], d["d" + n] = h.acq_grad(_acq_id(n), par, fmin)
                for k in (3, 7):
                    m, x = "rows%d " % k, np.ascontiguousarray(p["Xs"][:k])
                    d[m + "mean"], d[m + "var"], d[m + "dmdx"], d[m + "dvdx"] = h.predict_rows(x, True, grad=True)
                    d[m + "EI"], d[m + "dEI"] = h.acq_rows(x, _acq_id("EI"), 0.01, fmin, grad=True)
        finally:
            h.mean_set(None, None)
        return d


# ---- 5. the cost surface ---------------------------------------------------------------------------------------------------------------------
class Cost(Family):
    """gp_cost_set / gp_cost_rows with gradients.  Truth and tolerance: tests/_cost_truth.surface and the bound derived there (it
    already grows with |x / l|)."""
    roles = {"X0": COORD, "Xc": COORD, "Xs": COORD, "ls": LENGTH}
    methods = ("cost_set", "cost_rows")
    results = collections.OrderedDict([("logc", EXACT), ("dlogc", grad(1))])

    def __init__(self, cid):
        c = self.case = CT.CASES[cid]
        self.ard = c.ard
        self.name = "cost, case %s" % cid
        self.source = "_cost_truth case %s (%s, Nc = %d, D = %d, M = %d)" % (cid, c.fam, c.Nc, c.D, c.M)

    @functools.lru_cache(maxsize=None)
    def problem(self):
        p = CT.problem(self.case.id)
        rng = np.random.default_rng(3)                    # the handle's own data, of the surface's width: tests/test_gpu_cost.set_surface
        return dict(X0=rng.uniform(0, 1, (8, self.case.D)), Y0=rng.standard_normal((8, 1)), Xc=p.Xc, alpha=p.alpha, ls=p.ls_arg, Xs=p.Xs,
                    variance=p.variance)

    def lengthscales(self, p):
        ls = np.asarray(p["ls"], dtype=float)
        return [ls if ls.size == self.case.D else np.full(self.case.D, ls[0])]

    def _surface(self, p):
        c = self.case
        return CT.surface(c.fam, p["variance"], self.lengthscales(p)[0], p["Xc"], p["alpha"], c.shift, c.scale, p["Xs"])

    def truth(self, p):
        s = self._surface(p)
        return collections.OrderedDict([("logc", s[0]), ("dlogc", s[1])])

    def tolerance(self, p, t):
        s = self._surface(p)
        return dict(logc=np.asarray(s[2], dtype=float), dlogc=np.asarray(s[3], dtype=float))

    def device(self, h, p):
        c = self.case
        h.set_data(p["X0"], p["Y0"])
        h.cost_set(p["Xc"], p["alpha"], CT.KERNEL_IDS[c.fam], c.ard, p["variance"], p["ls"], c.shift, c.scale)
        try:
            logc, dlogc = h.cost_rows(p["Xs"], grad=True)
        finally:
            h.cost_set(None, None, 0, 0, 1.0, None)
        return collections.OrderedDict([("logc", logc), ("dlogc", dlogc)])


# ---- 6. posterior paths ----------------------------------------------------------------------------------------------------------------------
class Paths(Family):
    """gp_paths_set (the frequencies are omega_unit / l: they follow the scale by themselves), gp_paths_table over 300 candidates,
    gp_paths_argbest, gp_paths_rows with gradients on 8 locations.  Truth: tests/_paths_truth.evaluate; tolerance: combine's, whose
    prior-term bound already grows with |omega . x + b|."""
    roles = {"X": COORD, "Xs": COORD, "Xtab": COORD, "ls": LENGTH}
    methods = ("paths_set", "paths_rows")
    results = collections.OrderedDict([("table", EXACT), ("argbest", Index("table", -1)), ("rows", EXACT), ("drows", grad(1))])

    def __init__(self, cid):
        c = self.case = PT.CASES[cid]
        self.ard = c.ard
        self.name = "paths, case %s" % cid
        self.source = "_paths_truth case %s (%s, D = %d, N = %d, F = %d, S = %d)" % (cid, c.fam, c.D, c.N, c.F, c.S)

    @functools.lru_cache(maxsize=None)
    def problem(self):
        p = PT.problem(self.case.id)
        return dict(X=p.X, Y=p.Y, ls=p.ls_arg, Xs=p.Xs, Xtab=p.Xtab, draws=p.draws)

    def _path(self):
        return np.arange(PT.M_ROWS) % self.case.S

    def _both(self, p):
        c = self.case
        ls = self.lengthscales(p)[0]
        d = PT.sigma2(PT.NOISE)
        tab = PT.evaluate(c.fam, PT.VARIANCE, ls, d, p["X"], p["Y"], p["draws"], p["Xtab"], grad=False)
        rows = PT.evaluate(c.fam, PT.VARIANCE, ls, d, p["X"], p["Y"], p["draws"], p["Xs"], grad=True)
        return PT.combine(tab), PT.combine(rows)

    def truth(self, p):
        (val, _, _, _), (rv, _, rg, _) = self._both(p)
        path, idx = self._path(), np.arange(PT.M_ROWS)
        # (the argbest of the table's path 0 stands for all: one index per family result)
        return collections.OrderedDict([("table", val), ("argbest", np.argmin(val, axis=1)), ("rows", rv[path, idx]), ("drows", rg[path, idx])])

    def tolerance(self, p, t):
        (_, allow, _, _), (_, ra, _, rga) = self._both(p)
        path, idx = self._path(), np.arange(PT.M_ROWS)
        return dict(table=np.asarray(allow, dtype=float), rows=np.asarray(ra[path, idx], dtype=float), drows=np.asarray(rga[path, idx], dtype=float))

    def device(self, h, p):
        c = self.case
        h.set_data(p["X"], p["Y"])
        h.set_params(PT.FAMILY_ID[c.fam], int(c.ard), PT.VARIANCE, p["ls"], PT.NOISE)
        assert h.fit()[2] == 0.0
        h.paths_set(*p["draws"])
        try:
            h.set_candidates(p["Xtab"])
            d = collections.OrderedDict([("table", h.paths_table(PT.Y_MEAN, PT.Y_STD))])
            d["argbest"] = h.paths_argbest(-1, PT.Y_MEAN, PT.Y_STD)[0]
            d["rows"], d["drows"] = h.paths_rows(p["Xs"], self._path(), PT.Y_MEAN, PT.Y_STD, grad=True)
        finally:
            h.paths_set(None, None, None, None)
        return d


# ---- 7. append ---------------------------------------------------------------------------------------------------------------------------
class Append(Family):
    """gp_append under a fit whose candidates stay resident (they are not set again), then everything the handle serves.  Truth: the
    long-double GP of the grown data; tolerances: tests/test_gpu_append.check_against_oracle's."""
    roles = {"X": COORD, "Xs": COORD, "ls": LENGTH}
    methods = ("append",)
    results = collections.OrderedDict(
        [(n, EXACT) for n in ("lml", "logdet", "alpha", "chol", "mean", "var", "var0", "dvariance", "dnoise", "fmin", "EI")]
        + [("dlengthscale", grad(0)), ("dmdx", grad(1)), ("dvdx", grad(1)), ("rows3 mean", EXACT), ("rows3 dEI", grad(1))])

    def __init__(self, N0, k, rb):
        import _append_cases as AC
        i = [s for s, _ in AC.SHAPES].index((N0, k))
        self.fam, self.kid, self.ard = AC.KERNELS[(2 * i + rb) % len(AC.KERNELS)]
        self.N0, self.k, self.Dim, self.seed = N0, k, 2 if (i + rb) % 2 else 5, 31 * N0 + k + rb
        self.name = "append, %d + %d" % (N0, k)
        self.source = "_append_cases shape (%d, %d) as tests/test_gpu_append.py draws it (%s, D = %d, seed %d)" % (N0, k, self.fam, self.Dim, self.seed)

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import _append_cases as AC
        X, Y, Xs, ls, var, _ = AC.problem(self.seed, self.N0 + self.k, self.Dim, 1, self.fam, self.ard)
        return dict(X=X, Y=Y, Xs=Xs, ls=ls, variance=var)

    def truth(self, p):
        gp = _GP(self.fam, self.ard, p["variance"], p["ls"], 1e-2, p["X"], p["Y"])
        dvar, dls, dn = gp.all_gradients()[:3]
        mu, v0, v1, dm, dv = gp.at(_ld(p["Xs"]))
        ei, dei = _scores("EI", mu[:, 0], v1, dm[:, :, 0], dv, gp.fmin())
        return collections.OrderedDict([("lml", gp.lml), ("logdet", gp.logdet), ("alpha", gp.alpha), ("chol", gp.L), ("mean", mu),
                                        ("var", v1[:, None]), ("var0", v0[:, None]), ("dvariance", dvar), ("dnoise", dn), ("fmin", gp.fmin()),
                                        ("EI", ei), ("dlengthscale", dls), ("dmdx", dm), ("dvdx", dv), ("rows3 mean", mu[:3]),
                                        ("rows3 dEI", dei[:3])])

    def tolerance(self, p, t):
        m1 = lambda v, tol=1e-6: tol * max(1.0, float(np.max(np.abs(v))))   # noqa: E731
        sc = max(1.0, abs(float(t["dvariance"])), float(np.max(np.abs(t["dlengthscale"]))), abs(float(t["dnoise"])))
        return dict(lml=m1(t["lml"], 1e-8), logdet=m1(t["logdet"], 1e-8), alpha=m1(t["alpha"]), chol=1e-6 * float(np.max(np.abs(t["chol"]))),
                    mean=m1(t["mean"]), var=1e-6 * np.asarray(t["var"], dtype=float), var0=m1(t["var0"]) + 1e-9, dvariance=1e-6 * sc,
                    dlengthscale=1e-6 * sc, dnoise=1e-6 * sc, fmin=m1(t["fmin"]), EI=m1(t["EI"]), dmdx=m1(t["dmdx"]), dvdx=m1(t["dvdx"]),
                    **{"rows3 mean": m1(t["mean"]), "rows3 dEI": m1(t["rows3 dEI"], 1e-5)})

    def device(self, h, p):
        N0 = self.N0
        h.set_data(p["X"][:N0], 0.5 * p["Y"][:N0] + 0.3)       # every target changes with the append, as in the BO loop
        h.set_params(self.kid, int(self.ard), p["variance"], p["ls"], 1e-2)
        h.set_candidates(p["Xs"])
        h.fit()
        h.predict(True)
        lml, logdet = h.append(p["X"][N0:], p["Y"])
        d = collections.OrderedDict([("lml", np.array(lml)), ("logdet", np.array(logdet)), ("alpha", h.alpha()), ("chol", h.chol())])
        d["mean"], d["var"] = h.predict(True)
        d["var0"] = h.predict(False)[1]
        dv, d["dlengthscale"], dn = h.lml_grad(p["ls"].size)
        d["dvariance"], d["dnoise"] = np.array(dv), np.array(dn)
        d["dmdx"], d["dvdx"] = h.predict_grad()
        fmin = h.fmin()
        d["fmin"], d["EI"] = np.array(fmin), h.acq(_acq_id("EI"), 0.01, fmin)
        x = np.ascontiguousarray(p["Xs"][:3])
        d["rows3 mean"] = h.predict_rows(x, True)[0]
        d["rows3 dEI"] = h.acq_rows(x, _acq_id("EI"), 0.01, fmin, grad=True)[1]
        return d


# ---- 8. the sparse GP -------------------------------------------------------------------------------------------------------------------------
class Sparse(Family):
    """gp_sparse_set_inducing, gp_sparse_fit / _fit_grad (dZ with the inducing inputs' scale), gp_sparse_predict with gradients on
    130 rows, the full covariance of 9, the covariance between 8 locations and 130 resident points, and with one output the rows
    calls and the scored table.  Truth: tests/_sparse_ref.inference / predict and tests/_sparse_cov_ref in long double; tolerance:
    max(MULT x the float64 restatement's own error, 1e-13 x scale), MULT = 8 (tests/test_gpu_sparse_gp.py; 16 for the rows and
    scores, tests/test_gpu_sparse_acq.py)."""
    roles = {"X": COORD, "Z": COORD, "Xs": COORD, "X2": COORD, "ls": LENGTH, "Zb": COORD, "ls_b": LENGTH}
    VAR_B, NOISE_B = np.array([SR.VARIANCE, 0.8]), np.array([SR.NOISE, 3e-2])      # the two members of the batched fit
    methods = ("sparse_fit_grad_batch", "sparse_posterior_samples", "sparse_set_inducing", "sparse_predict", "sparse_set_candidates", "sparse_predict_rows", "sparse_mean_grad_rows",
               "sparse_acq_rows", "sparse_acq", "sparse_acq_argbest", "sparse_predict_full_cov", "sparse_cov_set_points", "sparse_cov_between")

    def __init__(self, case, fam, ard, first_offset):
        import _sparse_cov_ref  # noqa: F401
        self.case, self.fam, self.ard, self.first_offset = case, fam, ard, first_offset
        self.offset_note = "first offset %g instead of 1000: with 1000 2 Delta exceeds ten times the tolerance" % first_offset
        N, Mz, D, P = SR.CASES[case]
        self.P = P
        self.name = "sparse, case %s" % case
        self.source = "_sparse_ref case %s (N = %d, Mz = %d, D = %d, P = %d, %s), second points of _sparse_cov_ref" % (case, N, Mz, D, P, fam)
        r = [(n, EXACT) for n in ("lml", "woodbury_vector", "woodbury_inv", "dvariance", "dnoise", "mean", "var", "var0", "fmin", "cov",
                                  "between", "samples", "batch lml", "batch dvariance", "batch dnoise")]
        r += [("dlengthscale", grad(0)), ("dZ", grad(1)), ("dmdx", grad(1)), ("dvdx", grad(1)), ("batch dlengthscale", grad(1)),
              ("batch dZ", grad(2))]
        if P == 1:
            for k in (3, 8):
                r += [("rows%d mean" % k, EXACT), ("rows%d var" % k, EXACT), ("rows%d dmdx" % k, grad(1)), ("rows%d dvdx" % k, grad(1)),
                      ("rows%d dmdx alone" % k, grad(1)), ("rows%d EI" % k, EXACT), ("rows%d dEI" % k, grad(1))]
            r += [("EI", EXACT), ("dEI", grad(1)), ("EI argbest", Index("EI", -1))]
        self.results = collections.OrderedDict(r)

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import _sparse_cov_ref as SC
        X, Y, Z, Xs = SR.case_inputs(self.case)
        ls = SR.case_lengthscale(X.shape[1], self.ard)
        return dict(X=X, Y=Y, Z=Z, Xs=Xs, X2=SC.second_draw(self.case), ls=ls, Zb=np.stack([Z, Z]), ls_b=np.stack([ls, 1.5 * ls]),
                    normals=np.random.RandomState(3).standard_normal((4, 9)))

    def lengthscales(self, p):
        D = p["X"].shape[1]
        return [np.broadcast_to(np.asarray(l, dtype=float), (D,)) for l in p["ls_b"]]

    def _record(self, p, lin):
        import _sparse_cov_ref as SC
        f = SR.inference(self.fam, p["X"], p["Z"], p["Y"], SR.VARIANCE, p["ls"], self.ard, SR.NOISE, lin)
        assert f["jitter_kmm"] == 0.0 and f["jitter_b"] == 0.0
        mu, v1, dm, dv = SR.predict(f, p["Z"], p["Xs"], SR.NOISE, True, lin)
        v0 = SR.predict(f, p["Z"], p["Xs"], SR.NOISE, False, lin, grads=False)[1]
        t = collections.OrderedDict((n, f[n]) for n in ("lml", "woodbury_vector", "woodbury_inv", "dvariance", "dnoise"))
        fmin = np.min((f["kern"].K(np.asarray(p["X"], dtype=lin.dtype), np.asarray(p["Z"], dtype=lin.dtype)) @ f["woodbury_vector"])[:, 0])
        t["mean"], t["var"], t["var0"], t["fmin"] = mu, v1[:, None], v0[:, None], fmin
        t["cov"] = SC.full_cov(f, p["Z"], p["Xs"][:9], SR.NOISE, True, lin)[1]
        t["between"] = SC.cov_between(f, p["Z"], p["Xs"][:8], p["X2"], lin)
        t["samples"] = np.asarray(p["normals"], dtype=lin.dtype) @ np.asarray(lin.chol(t["cov"])[0], dtype=lin.dtype).T
        f1 = SR.inference(self.fam, p["X"], p["Zb"][1], p["Y"], self.VAR_B[1], p["ls_b"][1], self.ard, self.NOISE_B[1], lin)
        for n, q in (("batch lml", "lml"), ("batch dvariance", "dvariance"), ("batch dnoise", "dnoise")):
            t[n] = np.array([f[q], f1[q]], dtype=lin.dtype)
        t["dlengthscale"], t["dZ"], t["dmdx"], t["dvdx"] = f["dlengthscale"], f["dZ"], dm, dv
        t["batch dlengthscale"], t["batch dZ"] = np.array([f["dlengthscale"], f1["dlengthscale"]]), np.array([f["dZ"], f1["dZ"]])
        if self.P == 1:
            ei, dei = _scores("EI", mu[:, 0], v1, dm[:, :, 0], dv, fmin)
            for k in (3, 8):
                n = "rows%d " % k
                t[n + "mean"], t[n + "var"], t[n + "dmdx"], t[n + "dvdx"], t[n + "dmdx alone"] = mu[:k], v1[:k, None], dm[:k], dv[:k], dm[:k]
                t[n + "EI"], t[n + "dEI"] = ei[:k], dei[:k]
            t["EI"], t["dEI"], t["EI argbest"] = ei, dei, np.array(int(np.argmin(ei[:, 0])))
        return t

    def truth(self, p):
        return self._record(p, LD)

    def tolerance(self, p, t):
        with _pinned():
            o = self._record({k: (np.asarray(v, dtype=float) if isinstance(v, np.ndarray) else v) for k, v in p.items()}, F64)
        tol = {}
        for n, v in t.items():
            if isinstance(self.results[n], Index):
                continue
            e64, scale = MT.e64_of(o[n], v)
            tol[n] = max((16.0 if ("rows" in n or "EI" in n) else 8.0) * e64, 1e-13 * scale)
        tol["samples"] = _rel(t["samples"])               # tests/test_gpu_sparse_cov.py: the draws against Z C^T at 1e-6 of the largest
        return tol

    def device(self, h, p):
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id(self.fam), int(self.ard), SR.VARIANCE, p["ls"], SR.NOISE)
        h.sparse_set_inducing(p["Z"])
        d = collections.OrderedDict()
        lml0, jk, jb = h.sparse_fit()
        assert (jk, jb) == (0.0, 0.0)
        d["woodbury_vector"], d["woodbury_inv"] = h.sparse_posterior()
        lml, (dv, d["dlengthscale"], dn, d["dZ"]) = h.sparse_fit_grad(p["ls"].size)
        assert lml == lml0
        d["lml"], d["dvariance"], d["dnoise"] = np.array(lml), np.array(dv), np.array(dn)
        d["mean"], d["var"], d["dmdx"], d["dvdx"] = h.sparse_predict(p["Xs"], include_noise=True, grad=True)
        d["var0"] = h.sparse_predict(p["Xs"], include_noise=False)[1]
        fmin = h.sparse_fmin()
        d["fmin"] = np.array(fmin)
        d["cov"] = h.sparse_predict_full_cov(np.ascontiguousarray(p["Xs"][:9]), True)[1]
        h.sparse_cov_set_points(p["X2"])
        d["between"] = h.sparse_cov_between(np.ascontiguousarray(p["Xs"][:8]))
        _, d["samples"], jit = h.sparse_posterior_samples(np.ascontiguousarray(p["Xs"][:9]), p["normals"], include_noise=True)
        assert jit == 0.0
        (blml, bjk, bjb), (bdv, d["batch dlengthscale"], bdn, d["batch dZ"]), status = h.sparse_fit_grad_batch(p["Zb"], self.VAR_B, p["ls_b"],
                                                                                                              self.NOISE_B)
        assert not status.any() and not bjk.any() and not bjb.any()
        d["batch lml"], d["batch dvariance"], d["batch dnoise"] = blml, bdv, bdn
        if self.P == 1:
            ei = _acq_id("EI")
            for k in (3, 8):
                n, x = "rows%d " % k, np.ascontiguousarray(p["Xs"][:k])
                d[n + "mean"], d[n + "var"], d[n + "dmdx"], d[n + "dvdx"] = h.sparse_predict_rows(x, True, grad=True)
                d[n + "dmdx alone"] = h.sparse_mean_grad_rows(x)
                d[n + "EI"], d[n + "dEI"] = h.sparse_acq_rows(x, ei, 0.01, fmin, grad=True)
            h.sparse_set_candidates(p["Xs"])
            d["EI"], d["dEI"] = h.sparse_acq(ei, 0.01, fmin, grad=True)
            d["EI argbest"] = np.array(h.sparse_acq_argbest(ei, 0.01, fmin, -1)[0])
        return d


# ---- 9. input warping ------------------------------------------------------------------------------------------------------------------------
def kumaraswamy(X, a, b, lo, hi, cols, dtype=T):
    """tests/test_gpu_input_warped.py's closed form, column by column, on coordinates as given."""
    X = np.asarray(X, dtype=dtype)
    out = X.copy()
    for q in cols:
        u = (X[:, q] - np.asarray(lo, dtype=dtype)[q]) / (np.asarray(hi, dtype=dtype)[q] - np.asarray(lo, dtype=dtype)[q])
        out[:, q] = 1 - np.power(1 - np.power(u, dtype(a[q])), dtype(b[q]))
    return out


class InputWarp(Family):
    """gp_set_candidates_kumar: columns 0 and 2 are warped from [xmin, xmax] into [0, 1], where the model's data and lengthscales
    live and nothing moves; xmin and xmax follow the scale.  Column 1 is not warped: a coordinate like any other, scaled with its
    lengthscale.  Then the table entries on the warped candidates, and gp_fit_grad_x (what the warp's own gradients are chained
    from).  Truth: the closed form in long double and the long-double GP on its output; tolerances: the warp max(4 x NumPy's own
    error, 1e-15), the rest 1e-6 of the largest entry (tests/test_gpu_input_warped.py)."""
    name = "input warping"
    source = "tests/test_gpu_input_warped.py's table (130 rows, the first two on the bounds) and model (N = 300, D = 3, Mat52 ARD)"
    fam, COLS = "Mat52", (0, 2)
    WA, WB = np.array([0.6, 1.7, 1.0]), np.array([2.2, 0.8, 1.0])
    roles = {"Xs": COORD, "xmin": only(COORD, (0, 2), 3), "xmax": only(COORD, (0, 2), 3), "X": only(COORD, (1,), 3),
             "ls": only(LENGTH, (1,), 3), "Xw": only(COORD, (1,), 3), "ls_b": only(LENGTH, (1,), 3)}
    round_roles = {"Xs": only(COORD, (1,), 3), "X": only(COORD, (1,), 3), "Xw": only(COORD, (1,), 3)}      # x / l is formed in column 1 alone
    methods = ("set_candidates_kumar", "fit_grad_x", "fit_grad_x_batch")
    results = collections.OrderedDict([("warped", grad(1, +1)), ("mean", EXACT), ("var", EXACT), ("dL_dX", grad(1)), ("lml", EXACT),
                                       ("dlengthscale", grad(0)), ("batch lml", EXACT), ("batch dlengthscale", grad(1)),
                                       ("batch dL_dX", grad(2))])
    VAR_B, NOISE_B = np.array([1.3, 0.8]), np.array([1e-2, 3e-2])       # the two members of the batched fit over warped inputs

    def lengthscales(self, p):
        return [np.asarray(l, dtype=float) for l in p["ls_b"]]

    def result_exponents(self, k):
        """Only column 1 of the model's space moves: the warped table's column 1 is the raw coordinate (times 2^k_1), its columns
        0 and 2 and the gradients in them keep their bits."""
        return np.where(np.arange(3) == 1, k, 0)

    @functools.lru_cache(maxsize=None)
    def problem(self):
        Xs = np.random.default_rng(11).uniform(0, 1, (130, 3))
        Xs[0], Xs[1] = 0.0, 1.0
        rng = np.random.default_rng(12)
        X = rng.uniform(0, 1, (300, 3))
        Y = (np.sin(3 * X.sum(1)) + 0.1 * rng.standard_normal(300))[:, None]
        ls = np.array([0.4, 0.7, 1.1])
        return dict(X=X, Y=Y, Xs=Xs, ls=ls, xmin=np.zeros(3) - 1e-6, xmax=np.ones(3) + 1e-6, Xw=np.stack([X, X]), ls_b=np.stack([ls, 1.5 * ls]))

    def _warp(self, p, dtype):
        return kumaraswamy(p["Xs"], self.WA, self.WB, p["xmin"], p["xmax"], self.COLS, dtype)

    def truth(self, p):
        w = self._warp(p, T)
        gp = _GP(self.fam, True, 1.3, p["ls"], 1e-2, p["X"], p["Y"])
        mu, v0, v1, dm, dv = gp.at(w)
        dls, dX = gp.all_gradients()[1::2][:2]
        g1 = _GP(self.fam, True, self.VAR_B[1], p["ls_b"][1], self.NOISE_B[1], p["Xw"][1], p["Y"])
        dls1, dX1 = g1.all_gradients()[1::2][:2]
        return collections.OrderedDict([("warped", w), ("mean", mu), ("var", v1[:, None]), ("dL_dX", dX), ("lml", gp.lml),
                                        ("dlengthscale", dls), ("batch lml", np.array([gp.lml, g1.lml])),
                                        ("batch dlengthscale", np.array([dls, dls1])), ("batch dL_dX", np.array([dX, dX1]))])

    def tolerance(self, p, t):
        q = {k: (np.asarray(v, dtype=float) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        numpy_err = maxnorm(self._warp(q, np.float64)[:, self.COLS], kumaraswamy(q["Xs"], self.WA, self.WB, q["xmin"], q["xmax"], self.COLS, T)[:, self.COLS])
        gs = max(float(np.max(np.abs(t["dlengthscale"]))), 1.0)
        return {"warped": max(4.0 * numpy_err, 1e-15), "mean": _rel(t["mean"]), "var": 1e-6 * np.asarray(t["var"], dtype=float),
                "dL_dX": _rel(t["dL_dX"]), "lml": 1e-8 * abs(float(t["lml"])), "dlengthscale": 1e-6 * gs,
                "batch lml": 1e-8 * np.abs(np.asarray(t["batch lml"], dtype=float)),
                "batch dlengthscale": 1e-6 * np.maximum(np.abs(np.asarray(t["batch dlengthscale"], dtype=float)).max(1), 1.0)[:, None] * np.ones((2, 3)),
                "batch dL_dX": 1e-6 * np.abs(np.asarray(t["batch dL_dX"], dtype=float)).max(axis=(1, 2))[:, None, None] * np.ones(t["batch dL_dX"].shape)}

    def device(self, h, p):
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id(self.fam), 1, 1.3, p["ls"], 1e-2)
        (lml, _, jit), (_, dl, _), dX = h.fit_grad_x(3)
        assert jit == 0.0
        w = h.set_candidates_kumar(p["Xs"], [1, 0, 1], self.WA, self.WB, p["xmin"], p["xmax"], want_warped=True)
        mean, var = h.predict(True)
        (blml, _, bjit), (_, bdl, _), bdX, status = h.fit_grad_x_batch(p["Xw"], self.VAR_B, p["ls_b"], self.NOISE_B)
        assert not status.any() and not bjit.any()
        return collections.OrderedDict([("warped", w), ("mean", mean), ("var", var), ("dL_dX", dX), ("lml", np.array(lml)),
                                        ("dlengthscale", dl), ("batch lml", blml), ("batch dlengthscale", bdl), ("batch dL_dX", bdX)])


# ---- 10. joint expected improvement -----------------------------------------------------------------------------------------------------------
class JointEI(Family):
    """gp_qei_rows with the gradient and the joint posterior it factored.  The threshold t0 = fmin - par is the case's own (from
    the unit-cube truth: half the samples active) and does not move.  Truth: tests/_qei_truth.solve_case on the arrays as given;
    tolerances: tests/test_gpu_qei.py's -- the posterior at the rows' relative tolerance, the value at the adjoint's first-order
    allowance, the gradient at max(4 x the float64 restatement's own error, that relative tolerance of the largest entry)."""
    roles = {"X": COORD, "Xq": COORD, "ls": LENGTH}
    methods = ("qei_rows",)
    results = collections.OrderedDict([("mean", EXACT), ("cov", EXACT), ("value", EXACT), ("gradient", grad(1))])

    def __init__(self, cid):
        import _qei_truth as QT
        c = self.case = QT.CASES[cid]
        self.ard = c.ard
        self.name = "qEI, case %s" % cid
        self.source = "_qei_truth case %s (%s, N = %d, D = %d, q = %d, S = %d)" % (cid, c.fam, c.N, c.D, c.q, c.S)

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import _qei_truth as QT
        p = QT.problem(self.case.id)
        return dict(X=p.X, Y=p.Y, ls=p.ls_arg, Xq=p.Xq, Z=p.Z, t0=QT.truth(self.case.id).t0)

    def _solve(self, p, dtype):
        import _qei_truth as QT
        q = QT.Problem(self.case, p["X"], p["Y"], self.lengthscales(p)[0], p["ls"], p["Xq"], p["Z"])
        return QT.solve_case(self.case, q, 0.0, dtype, p["t0"])

    def truth(self, p):
        tr = self._solve(p, T).truth
        return collections.OrderedDict([("mean", tr.mean), ("cov", tr.cov), ("value", -tr.value), ("gradient", -tr.grad)])

    def tolerance(self, p, t):
        import _qei_truth as QT
        sv = self._solve(p, T)
        with _pinned():
            f64 = self._solve({k: (np.asarray(v, dtype=float) if isinstance(v, np.ndarray) else v) for k, v in p.items()}, np.float64)
        m_norm = float(np.max(np.abs((sv.truth.mean - T(QT.Y_MEAN)) / T(QT.Y_STD))))
        tol_m, tol_S = QT.tolerances(self.case.noise, m_norm)
        g = sv.truth.grad
        return dict(mean=tol_m, cov=tol_S, value=sv.allowance,
                    gradient=max(4 * maxnorm(f64.truth.grad, g), QT.rel_tol(self.case.noise) * float(np.max(np.abs(g)))))

    def device(self, h, p):
        import _qei_truth as QT
        c = self.case
        h.set_data(p["X"], p["Y"])
        h.set_params(QT.FAMILY_ID[c.fam], int(c.ard), QT.VARIANCE, p["ls"], c.noise)
        assert h.fit()[2] == 0.0
        h.qei_set(p["Z"])
        value, g, mean, cov = h.qei_rows(p["Xq"], QT.PAR, p["t0"] + QT.PAR, QT.Y_MEAN, QT.Y_STD, grad=True, posterior=True)
        return collections.OrderedDict([("mean", mean), ("cov", cov), ("value", np.array(value)), ("gradient", g)])


# ---- 11. feasibility ---------------------------------------------------------------------------------------------------------------------------
class Feasibility(Family):
    """gp_feas_rows with gradients, gp_feas_table over the scored handle's candidates, gp_acq_rows_feas (EI times the probability
    of feasibility, with gradients): the scored model and K constraint models, each with its own snapshot of inputs, all moved
    together.  The bounds put z near 0 at location k mod M on the unit-cube problem and stay.  Truth: the long-double GP of every
    model folded by tests/_feas_truth.fold; tolerance: tests/test_gpu_feas.py's end-to-end one -- fold's rounding bound plus the
    rows' posterior tolerance propagated through the fold."""
    roles = {"X": COORD, "Xc": COORD, "Xs": COORD, "Xtab": COORD, "ls": LENGTH}
    methods = ("feas_table", "acq_rows_feas", "FeasPack.rows")
    results = collections.OrderedDict([("logF", EXACT), ("dlogF", grad(1)), ("table", EXACT), ("EI x F", EXACT), ("d(EI x F)", grad(1))])

    def __init__(self, cid, first_offset=OFFSETS[0]):
        import _feas_truth as FT
        c = self.case = FT.CASES[cid]
        self.ard, self.first_offset = c.ard, first_offset
        if first_offset != OFFSETS[0]:
            self.offset_note = "first offset %g instead of 1000: with 1000 2 Delta exceeds ten times the tolerance" % first_offset
        self.name = "feasibility, case %s" % cid
        self.source = "_feas_truth case %s (%s, D = %d, K = %d, Nc = %s, N = 200, M = %d, table of %d)" % (cid, c.fam, c.D, c.K, c.Nc, c.M, c.Mtab)

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import _feas_truth as FT
        p = FT.problem(self.case.id)
        q = dict(X=p.X, Y=p.Y, Xc=p.Xc, C=p.C, ls=p.ls_arg, Xs=p.Xs, Xtab=p.Xtab, variance=p.variance, noise=p.noise, c_mean=p.c_mean, c_std=p.c_std)
        mean, var = self._posteriors(q, q["Xs"])[:2]
        m = np.asarray(mean, dtype=float) * p.c_std[:, None] + p.c_mean[:, None]
        sd = np.sqrt(np.maximum(np.asarray(var, dtype=float) * p.c_std[:, None] ** 2, 1e-10))
        q["bounds"] = FT.bounds_for(self.case.id, 0.0, m, sd)
        return q

    def _posteriors(self, p, x):
        """(mean, var with noise [K, M], dmdx, dvdx [K, M, D]) of the constraint models at x, long double."""
        c, out = self.case, []
        for k in range(c.K):
            mu, _, v1, dm, dv = _GP(c.fam, c.ard, p["variance"], p["ls"], p["noise"][k], p["Xc"][k], p["C"][k]).at(_ld(x))
            out.append((mu[:, 0], v1, dm[:, :, 0], dv))
        return tuple(np.stack(a) for a in zip(*out))

    def _all(self, p):
        import _feas_truth as FT
        c = self.case
        post = self._posteriors(p, p["Xs"])
        g = FT.fold(*post, p["c_mean"], p["c_std"], p["bounds"])
        tab = FT.fold(*self._posteriors(p, p["Xtab"])[:2], None, None, p["c_mean"], p["c_std"], p["bounds"])
        gp = _GP(c.fam, c.ard, p["variance"], p["ls"], 1e-2, p["X"], p["Y"])
        mu, _, v1, dm, dv = gp.at(_ld(p["Xs"]))
        f0, df0 = _scores("EI", mu[:, 0], v1, dm[:, :, 0], dv, gp.fmin())
        return post, g, tab, np.asarray(f0[:, 0], dtype=T), np.asarray(df0, dtype=T)

    def truth(self, p):
        post, g, tab, f0, df0 = self._all(p)
        F = np.exp(g.logF)
        return collections.OrderedDict([("logF", g.logF), ("dlogF", g.dlogF), ("table", tab.logF), ("EI x F", (f0 * F)[:, None]),
                                        ("d(EI x F)", df0 * F[:, None] + (f0 * F)[:, None] * g.dlogF)])

    def tolerance(self, p, t):
        import _feas_truth as FT
        post, g, tab, f0, df0 = self._all(p)

        def ptol(post, grads=True):
            mean, var = np.asarray(post[0], dtype=float), np.asarray(post[1], dtype=float)
            sd = np.sqrt(np.maximum(var, 0.0))
            out = [1e-6 * np.maximum(1.0, np.abs(mean)), 1e-6 * sd + 1e-12]
            if grads:
                dm, dv = np.asarray(post[2], dtype=float), np.asarray(post[3], dtype=float)
                out += [np.broadcast_to(1e-6 * np.maximum(np.abs(dm).max(axis=(1, 2)), 1e-3)[:, None, None], dm.shape),
                        np.full(dv.shape, 1e-6 * p["variance"])]
            return out

        tl, td = FT.propagate(g, p["c_std"], *ptol(post), post[2], post[3])
        tl, td = tl + g.bound_logF, td + g.bound_dlogF
        ttab = FT.propagate(tab, p["c_std"], *ptol(self._posteriors(p, p["Xtab"]), False))[0] + tab.bound_logF
        F, want = np.exp(g.logF), np.abs(f0 * np.exp(g.logF))
        ta = 1e-5 * np.abs(f0).max() * F + want * tl
        tda = (1e-5 * np.abs(df0).max() * F)[:, None] + np.abs(df0) * (F * tl)[:, None] + want[:, None] * (tl[:, None] * np.abs(g.dlogF) + td)
        f = lambda a: np.asarray(a, dtype=float)   # noqa: E731
        return {"logF": f(tl), "dlogF": f(td), "table": f(ttab), "EI x F": f(ta)[:, None], "d(EI x F)": f(tda)}

    def device(self, h, p):
        from gaussian_process_optimization_amd import _lib
        c = self.case
        kid = _kernel_id(c.fam)
        cons = []
        try:
            for k in range(c.K):
                hk = _lib.Handle(0)
                cons.append(hk)
                hk.set_option("emulate_fp64", 0)
                hk.set_data(p["Xc"][k], p["C"][k])
                hk.set_params(kid, int(c.ard), p["variance"], p["ls"], p["noise"][k])
                assert hk.fit()[2] == 0.0
            h.set_data(p["X"], p["Y"])
            h.set_params(kid, int(c.ard), p["variance"], p["ls"], 1e-2)
            h.fit()
            pack = _lib.FeasPack(cons, p["bounds"], p["c_mean"], p["c_std"])
            d = collections.OrderedDict()
            d["logF"], d["dlogF"] = pack.rows(p["Xs"], grad=True)
            h.set_candidates(p["Xtab"])
            h.feas_table(pack)
            d["table"] = h.feas_get_table()
            h.feas_table(None)
            d["EI x F"], d["d(EI x F)"] = h.acq_rows_feas(pack, p["Xs"], _acq_id("EI") | _lib.GP_ACQ_TIMES_FEAS, 0.01, h.fmin(), grad=True)
        finally:
            for hk in cons:
                hk.close()
        return d


# ---- 12. max-value entropy search -------------------------------------------------------------------------------------------------------------
class MaxValue(Family):
    """gp_mes_bracket and gp_mes_logsurv over a latent table of 300, and GP_ACQ_MES with gradients through gp_acq_rows on 8 rows
    (fused, wide) and through the table entries on 9.  The samples of the minimum (g = 0 at location k mod 9) and the three trial
    values (the quartile points of the bracket) are placed on the unit-cube problem and stay.  Truth: the long-double GP through
    tests/_mes_truth.score / logsurv; tolerance: tests/test_gpu_mes.py's end-to-end one -- the rule's rounding bound plus the rows'
    posterior tolerance propagated through it; the bracket's ends move by at most y_std (d_mean + 8 d_sd) of that tolerance."""
    roles = {"X": COORD, "Xs": COORD, "Xtab": COORD, "ls": LENGTH}
    methods = ()                # (mes_set, mes_logsurv and mes_bracket take values of y; the coordinates are the resident ones)
    results = collections.OrderedDict([("bracket", EXACT), ("logsurv", EXACT), ("rows MES", EXACT), ("rows dMES", grad(1)), ("table MES", EXACT),
                                       ("table dMES", grad(1))])

    def __init__(self, cid):
        import _mes_truth as ME
        c = self.case = ME.CASES[cid]
        self.ard = c.ard
        self.name = "MES, case %s" % cid
        self.source = "_mes_truth case %s (%s, D = %d, N = %d, K = %d), the first 300 rows of its table" % (cid, c.fam, c.D, c.N, c.K)

    def _gp(self, p):
        import _mes_truth as ME
        return _GP(self.case.fam, self.ard, p["variance"], p["ls"], ME.NOISE, p["X"], p["Y"])

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import _mes_truth as ME
        p = ME.problem(self.case.id)
        q = dict(X=p.X, Y=p.Y, ls=p.ls_arg, Xs=p.Xs, Xtab=p.Xtab[:300], variance=p.variance)
        gp = self._gp(q)
        mu, _, v1, _, _ = gp.at(_ld(q["Xs"]))
        m, sd = np.asarray(mu[:, 0], dtype=float) * ME.Y_STD + ME.Y_MEAN, np.sqrt(np.maximum(np.asarray(v1, dtype=float) * ME.Y_STD ** 2, 1e-10))
        q["ystar"] = ME.ystar_for(self.case.id, 0.0, m, sd)
        lo, hi = self._bracket(gp, q)[0]
        q["y"] = float(lo) + (float(hi) - float(lo)) * np.array([0.25, 0.5, 0.75])
        return q

    def _bracket(self, gp, p):
        import _mes_truth as ME
        mu, v0, _, _, _ = gp.at(_ld(p["Xtab"]))
        m, s = mu[:, 0] * T(ME.Y_STD) + T(ME.Y_MEAN), np.sqrt(np.maximum(v0 * T(ME.Y_STD) ** 2, T(1e-10)))
        return np.array([(m - 8 * s).min(), (m + 8 * s).min()]), (mu[:, 0], v0)

    def _all(self, p):
        import _mes_truth as ME
        gp = self._gp(p)
        br, (lm, lv) = self._bracket(gp, p)
        mu, _, v1, dm, dv = gp.at(_ld(p["Xs"]))
        post = (mu[:, 0], v1, dm[:, :, 0], dv)
        return br, (lm, lv), ME.logsurv(lm, lv, ME.Y_MEAN, ME.Y_STD, p["y"]), post, ME.score(*post, p["ystar"], ME.Y_MEAN, ME.Y_STD)

    def truth(self, p):
        br, _, ls, _, sc = self._all(p)
        return collections.OrderedDict([("bracket", br), ("logsurv", ls.value), ("rows MES", -sc.alpha[:8, None]), ("rows dMES", -sc.dalpha[:8]),
                                        ("table MES", -sc.alpha[:, None]), ("table dMES", -sc.dalpha)])

    def tolerance(self, p, t):
        import _mes_truth as ME
        br, (lm, lv), ls, post, sc = self._all(p)
        f = lambda a: np.asarray(a, dtype=float)   # noqa: E731
        mean, var, dm, dv = (f(a) for a in post)
        ptol = (1e-6 * np.maximum(1.0, np.abs(mean)), 1e-6 * np.sqrt(np.maximum(var, 0.0)) + 1e-12,
                np.full(dm.shape, 1e-6 * max(np.abs(dm).max(), 1e-3)), np.full(dv.shape, 1e-6 * p["variance"]))
        tl, td = ME.propagate(sc, ME.Y_STD, *ptol)
        ta, tda = f(tl + sc.bound_alpha), f(td + sc.bound_dalpha)
        d_mean, d_sd = 1e-6 * np.maximum(1.0, np.abs(f(lm))), 1e-6 * np.sqrt(np.maximum(f(lv), 0.0)) + 1e-12
        tls = f(ls.bound + ME.propagate_logsurv(lm, lv, ME.Y_MEAN, ME.Y_STD, p["y"], d_mean, d_sd))
        return {"bracket": float(np.max(ME.Y_STD * (d_mean + 8 * d_sd))), "logsurv": tls, "rows MES": ta[:8, None], "rows dMES": tda[:8],
                "table MES": ta[:, None], "table dMES": tda}

    def device(self, h, p):
        import _mes_truth as ME
        from gaussian_process_optimization_amd import _lib
        c, mes, ym, ys = self.case, _lib.GP_ACQ_MES, ME.Y_MEAN, ME.Y_STD
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id(c.fam), int(c.ard), p["variance"], p["ls"], ME.NOISE)
        assert h.fit()[2] == 0.0
        h.mes_set(p["ystar"])
        try:
            d = collections.OrderedDict()
            h.set_candidates(p["Xtab"])
            d["bracket"] = np.array(h.mes_bracket(8.0, include_noise=False, y_mean=ym, y_std=ys))
            d["logsurv"] = h.mes_logsurv(p["y"], include_noise=False, y_mean=ym, y_std=ys)
            d["rows MES"], d["rows dMES"] = h.acq_rows(np.ascontiguousarray(p["Xs"][:8]), mes, 0.0, 0.0, ym, ys, grad=True)
            h.set_candidates(p["Xs"])
            d["table MES"], d["table dMES"] = h.acq_grad(mes, 0.0, 0.0, ym, ys)
        finally:
            h.mes_set(None)
        return d


# ---- 13. the ensemble -------------------------------------------------------------------------------------------------------------------------
class Ensemble(Family):
    """gp_ens_fit over S = 3 members (every member's lengthscales follow the scale), gp_ens_predict_rows with gradients and
    gp_ens_acq_rows (EI integrated over the members, with gradients) on eight locations.  Truth: the long-double GP per member, the
    oracle's rule averaged; tolerance: tests/test_gpu_ensemble_sizes.py's max(64 e64, 1e-13 max(1, Npad / 384) scale), e64 the
    pinned float64 oracle's own error on the same arrays."""
    name = "ensemble"
    source = "_ens_truth case t (rbf, ARD, N = 130, D = 2), its first three of 64 members, its eight points"
    fam, S = "rbf", 3
    roles = {"X": COORD, "Xs": COORD, "ls": LENGTH, "ls_members": LENGTH}
    methods = ("ens_fit", "ens_predict_rows", "ens_acq_rows")
    results = collections.OrderedDict([(n, EXACT) for n in ("lml", "logdet", "jitter", "fmin", "mean", "var", "EI")]
                                      + [("dmdx", grad(2)), ("dvdx", grad(2)), ("dEI", grad(1))])

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import _ens_truth as ET
        X, Y, ls = ET.problem("t")
        var, lsm, noise = ET.members("t")
        return dict(X=X, Y=Y, Xs=ET.points("t"), ls=ls, ls_members=lsm[:self.S].copy(), var_members=var[:self.S].copy(),
                    noise_members=noise[:self.S].copy())

    def lengthscales(self, p):
        return [np.asarray(l, dtype=float) for l in p["ls_members"]]

    def _record(self, p, double):
        rec = []
        for z in range(self.S):
            var, ls, noise = float(p["var_members"][z]), p["ls_members"][z], float(p["noise_members"][z])
            if double:
                X, x = np.asarray(p["X"], dtype=float), np.asarray(p["Xs"], dtype=float)
                gp = O.OracleGP(X, p["Y"], KF.make(self.fam, X.shape[1], var, ls, True, direct=True), noise)
                mu, v0 = gp.predict_noiseless(x)
                dm, dv = gp.predictive_gradients(x)
                post = gp.posterior
                rec.append((post["lml"], post["logdet"], 0.0, float(gp.predict(X)[0].min()), mu[:, 0], v0[:, 0] + noise, dm[:, :, 0], dv))
            else:
                gp = _GP(self.fam, True, var, ls, noise, p["X"], p["Y"])
                mu, _, v1, dm, dv = gp.at(_ld(p["Xs"]))
                rec.append((gp.lml, gp.logdet, T(0), gp.fmin(), mu[:, 0], v1, dm[:, :, 0], dv))
        t = collections.OrderedDict()
        for i, n in enumerate(("lml", "logdet", "jitter", "fmin", "mean", "var", "dmdx", "dvdx")):
            t[n] = np.array([r[i] for r in rec], dtype=np.float64 if double else T)
        sc = [_scores("EI", r[4], r[5], r[6], r[7], r[3]) for r in rec]
        t["EI"] = sum(np.asarray(v, dtype=T) for v, _ in sc) / self.S
        t["dEI"] = sum(np.asarray(g, dtype=T) for _, g in sc) / self.S
        return t

    def truth(self, p):
        return self._record(p, False)

    def tolerance(self, p, t):
        import _ens_truth as ET
        with _pinned():
            o = self._record(p, True)
        tol = {}
        for n, v in t.items():
            e64, scale = ET.e64_of(o[n], v)
            tol[n] = max(ET.MULT * e64, ET.floor_n(p["X"].shape[0]) * scale)
        tol["jitter"] = 0.0
        return tol

    def device(self, h, p):
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id(self.fam), 1, FS.VAR, p["ls"], FS.NOISE)
        d = collections.OrderedDict()
        d["lml"], d["logdet"], d["jitter"], d["fmin"] = h.ens_fit(p["var_members"], p["ls_members"], p["noise_members"])
        d["mean"], d["var"], d["dmdx"], d["dvdx"] = h.ens_predict_rows(p["Xs"], True, grad=True)
        d["EI"], d["dEI"] = h.ens_acq_rows(p["Xs"], _acq_id("EI"), 0.01, grad=True)
        return d


# ---- 14. entropy search -----------------------------------------------------------------------------------------------------------------------
class EntropySearch(Family):
    """gp_es_set_representers (their joint posterior), gp_es_acq over 30 candidates, gp_es_acq_argbest and gp_es_acq_rows on 8.
    The belief over the 17 representers (tests/_es_truth.belief on the unit-cube truth's posterior, u and the 7 quantiles as
    tests/test_gpu_entropy_search.py draws them) is an input and stays.  Truth: the long-double GP's covariances through
    tests/_es_truth.score; tolerance: that test's 1e-9 of the largest reference entry."""
    name = "entropy search"
    source = "_family_shapes case j's model; representers: its candidates 40 .. 56, scored: its first 30"
    fam, R, YS = "Mat52", 17, 2.5
    roles = {"X": COORD, "Xs": COORD, "Xr": COORD, "ls": LENGTH}
    methods = ("es_set_representers", "es_acq_rows")
    results = collections.OrderedDict([("mu", EXACT), ("cov", EXACT), ("table", EXACT), ("argbest", Index("table", -1)), ("rows", EXACT)])

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import _es_truth as ES
        from scipy.stats import norm
        d = FAMILIES["dense anchor, Mat52 ARD"].problem()
        p = dict(X=d["X"], Y=d["Y"], ls=d["ls"], Xr=d["Xs"][40:40 + self.R].copy(), Xs=d["Xs"][:30].copy())
        mu, cov = self._representers(self._gp(p), p)
        cov = np.maximum(np.asarray(cov, dtype=float), 1e-10)
        p["logP"], p["dMu"], p["dSigma"], p["dMuMu"] = ES.belief(np.asarray(mu, dtype=float), cov)
        p["u"] = -np.random.default_rng(50 + self.R).uniform(0.5, 6.0, self.R)
        p["W"] = norm.ppf(np.linspace(1. / 8, 1 - 1. / 8, 7))
        H, idx = p["dMuMu"], [(a, b) for a in range(self.R) for b in range(a + 1)]
        Tm = np.zeros((self.R, self.R, self.R))          # entropy_search.quadratic_forms, restated: the packed rows unpacked
        for n, (a, b) in enumerate(idx):
            Tm[:, a, b] = p["dSigma"][:, n]
        p["Q"] = 0.25 * (H + H.transpose(0, 2, 1)) - 0.5 * (Tm + Tm.transpose(0, 2, 1))
        return p

    def _gp(self, p):
        return _GP(self.fam, True, FS.VAR, p["ls"], FS.NOISE, p["X"], p["Y"])

    def _representers(self, gp, p):
        Xr = _ld(p["Xr"])
        kr = gp.kern.K(Xr, gp.X)
        self._wr = LD.solve(gp.L, kr.T, 0)
        cov = gp.kern.K(Xr) - self._wr.T @ self._wr + gp.noise * np.eye(self.R, dtype=T)
        return (kr @ gp.alpha)[:, 0] * T(self.YS), cov * T(self.YS) ** 2

    def truth(self, p):
        import _es_truth as ES
        gp = self._gp(p)
        mu, cov = self._representers(gp, p)
        Xs = _ld(p["Xs"])
        ks = gp.kern.K(Xs, gp.X)
        ws = LD.solve(gp.L, ks.T, 0)
        var0 = gp.kern.variance - np.sum(ws * ws, axis=0)
        C = gp.kern.K(_ld(p["Xr"]), Xs) - self._wr.T @ ws
        ys2 = T(self.YS) ** 2
        out = []
        for j in range(Xs.shape[0]):
            m = C[:, j] * ys2 / np.sqrt(np.maximum(var0[j] * ys2, T(1e-10)))
            out.append(ES.score(m, p["logP"], p["u"], p["dMu"], ES.det_reference_style(m, p["dSigma"], p["dMuMu"]), p["W"]))
        tab = np.array(out, dtype=T).reshape(-1, 1)
        return collections.OrderedDict([("mu", mu), ("cov", cov), ("table", tab), ("argbest", np.array(int(np.argmin(tab[:, 0])))), ("rows", tab[:8])])

    def tolerance(self, p, t):
        return dict(mu=_rel(t["mu"], 1e-9), cov=_rel(t["cov"], 1e-9), table=_rel(t["table"], 1e-9), rows=_rel(t["table"], 1e-9))

    def device(self, h, p):
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id(self.fam), 1, FS.VAR, p["ls"], FS.NOISE)
        assert h.fit()[2] == 0.0
        d = collections.OrderedDict()
        d["mu"], d["cov"] = h.es_set_representers(p["Xr"], 0.0, self.YS)
        h.es_set_belief(p["logP"], p["u"], p["dMu"], p["Q"], p["W"])
        h.set_candidates(p["Xs"])
        d["table"] = h.es_acq(self.YS)
        d["argbest"] = np.array(h.es_acq_argbest(-1, self.YS)[0])
        d["rows"] = h.es_acq_rows(np.ascontiguousarray(p["Xs"][:8]), self.YS)
        return d


# ---- 15. expected hypervolume improvement --------------------------------------------------------------------------------------------------------
class Hypervolume(Family):
    """gp_ehvi_rows with gradients, gp_ehvi_table over 130 candidates and gp_ehvi_argbest: K objective models over one set of
    inputs.  The decomposition (the case's front placed so that location 0 lies inside the non-dominated region of the unit-cube
    problem) lives in the objectives' space and stays.  The cases of tests/_ehvi_truth.py all have N = 120: none crosses a row
    tile.  Truth: the long-double GP of every objective through tests/_ehvi_truth.ehvi; tolerance: tests/test_gpu_ehvi.py's
    end-to-end one -- the fold's rounding bound plus the rows' posterior tolerance propagated through it."""
    roles = {"X": COORD, "Xs": COORD, "Xtab": COORD, "ls": LENGTH}
    methods = ("EhviPack.rows",)
    results = collections.OrderedDict([("rows", EXACT), ("drows", grad(1)), ("table", EXACT), ("argbest", Index("table", -1))])

    def __init__(self, cid):
        import _ehvi_truth as EH
        c = self.case = EH.CASES[cid]
        self.ard = c.ard
        self.name = "EHVI, case %s" % cid
        self.source = "_ehvi_truth case %s (%s, D = %d, K = %d, N = 120, M = %d), the first 130 rows of its table" % (cid, c.fam, c.D, c.K, c.M)

    def _posteriors(self, p, x):
        c, out = self.case, []
        for k in range(c.K):
            mu, _, v1, dm, dv = _GP(c.fam, c.ard, p["variance"], p["ls"], p["noise"][k], p["X"], p["Y"][:, k:k + 1]).at(_ld(x))
            out.append((mu[:, 0], v1, dm[:, :, 0], dv))
        return tuple(np.stack(a) for a in zip(*out))

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import _ehvi_truth as EH
        p = EH.problem(self.case.id)
        q = dict(X=p.X, Y=p.Y, ls=p.ls_arg, Xs=p.Xs, Xtab=p.Xtab[:130], variance=p.variance, noise=p.noise, y_mean=p.y_mean, y_std=p.y_std)
        mean, var = (np.asarray(a, dtype=float) for a in self._posteriors(q, q["Xs"][:1])[:2])
        front, ref = EH.placed_front(self.case.id, "inside", mean[:, 0] * p.y_std + p.y_mean, np.sqrt(np.maximum(var[:, 0] * p.y_std ** 2, 1e-10)))
        q["levels"], q["lo"], q["hi"] = EH.cells_of(front, ref)
        return q

    def _all(self, p):
        import _ehvi_truth as EH
        post, tab = self._posteriors(p, p["Xs"]), self._posteriors(p, p["Xtab"])
        return (post, EH.ehvi(*post, p["y_mean"], p["y_std"], p["levels"], p["lo"], p["hi"]), tab,
                EH.ehvi(*tab[:2], None, None, p["y_mean"], p["y_std"], p["levels"], p["lo"], p["hi"]))

    def truth(self, p):
        _, t, _, tt = self._all(p)
        return collections.OrderedDict([("rows", -t.value[:, None]), ("drows", -t.grad), ("table", -tt.value[:, None]),
                                        ("argbest", np.array(int(np.argmin(-tt.value))))])

    def tolerance(self, p, t):
        import _ehvi_truth as EH
        post, tr, tab, tt = self._all(p)

        def ptol(post, grads=True):
            mean, var = np.asarray(post[0], dtype=float), np.asarray(post[1], dtype=float)
            out = [1e-6 * np.maximum(1.0, np.abs(mean)), 1e-6 * np.sqrt(np.maximum(var, 0.0)) + 1e-12]
            if grads:
                dm, dv = np.asarray(post[2], dtype=float), np.asarray(post[3], dtype=float)
                out += [np.broadcast_to(1e-6 * np.maximum(np.abs(dm).max(axis=(1, 2)), 1e-3)[:, None, None], dm.shape),
                        np.full(dv.shape, 1e-6 * p["variance"])]
            return out

        tv, tg = EH.propagate(tr, p["y_std"], p["lo"], p["hi"], *ptol(post), post[2], post[3])
        ttab = EH.propagate(tt, p["y_std"], p["lo"], p["hi"], *ptol(tab, False))[0]
        f = lambda a: np.asarray(a, dtype=float)   # noqa: E731
        return dict(rows=f(tv + tr.bound_value)[:, None], drows=f(tg + tr.bound_grad), table=f(ttab + tt.bound_value)[:, None])

    def device(self, h, p):
        from gaussian_process_optimization_amd import _lib
        c = self.case
        hs = [h]
        try:
            for k in range(c.K):
                if k:
                    hs.append(_lib.Handle(0))
                    hs[k].set_option("emulate_fp64", 0)
                hs[k].set_data(p["X"], p["Y"][:, k:k + 1])
                hs[k].set_params(_kernel_id(c.fam), int(c.ard), p["variance"], p["ls"], p["noise"][k])
                assert hs[k].fit()[2] == 0.0
            pack = _lib.EhviPack(hs, p["y_mean"], p["y_std"])
            pack.set_cells(p["levels"], p["lo"], p["hi"])
            d = collections.OrderedDict()
            d["rows"], d["drows"] = pack.rows(p["Xs"], grad=True)
            h.set_candidates(p["Xtab"])
            d["table"] = pack.table()
            d["argbest"] = np.array(pack.argbest(-1)[0])
            pack.clear()
        finally:
            for hk in hs[1:]:
                hk.close()
        return d


# ---- the table ------------------------------------------------------------------------------------------------------------------------
FAMILIES = collections.OrderedDict()


def _add(f):
    FAMILIES[f.name] = f
    return f


_add(Dense("Mat52", True))
_add(Dense("Exponential", False))
_add(LocalPenalisation())
_add(Gower())
_add(MeanFunction("d"))
_add(MeanFunction("e"))
_add(Cost("d"))
_add(Cost("c"))
_add(Paths("a"))
_add(Paths("d"))
_add(Append(120, 9, 1))
_add(Append(250, 28, 0))
_add(Sparse("S2", "Mat52", True, 250.0))          # (1000: woodbury_inv at 6.0 of the condition, 500: 1.9)
_add(InputWarp())
_add(JointEI("b"))
_add(JointEI("a"))
_add(Feasibility("b"))
_add(Feasibility("d"))
_add(MaxValue("e"))
_add(MaxValue("b"))
_add(Ensemble())
_add(EntropySearch())
_add(Hypervolume("f"))
_add(Hypervolume("d"))
_add(Sparse("S3", "Exponential", False, 31.25))   # (1000: dZ at 30 of the condition, 125: 1.4, 62.5: 1.6)


# ---- the residue path: part 1 alone --------------------------------------------------------------------------------------------------------
class ResiduePath(object):
    """Option emulate_fp64 = 1 moves the trailing update of the factorisation and the candidate solve onto the int8 matrix cores
    (csrc/rns.hip) -- where there is more than one panel to update.  With the default panel width of six tiles that needs more than
    768 rows: at the N <= 300 of the families above the option changes no kernel (one panel; solve_rows_rns ends after the fp64
    panel solve), and the sparse and batched entries are always true fp64, so none of them is run a second time with it.  This
    case has 1024 rows, two panels.  Its fixed-point scale is taken from the matrix entries, which the scaling does not move, so
    part 1 holds here as well; tests/test_gpu_domains.py runs it with the residue GEMM's launches counted.  No part 2: a
    long-double truth of 1024 rows with its Delta does not fit a test of a few seconds, and tests/test_gpu_emulation.py holds
    the path to the fp64 one."""
    name = "residue path"
    source = "_ens_truth case q (rbf, one lengthscale, N = 1024, D = 2: eight tiles, panels of six and two), its 130-row table"
    ard = False
    roles = {"X": COORD, "Xs": COORD, "ls": LENGTH}
    results = collections.OrderedDict([(n, EXACT) for n in ("lml", "logdet", "alpha", "mean", "var")] + [("dmdx", grad(1)), ("dvdx", grad(1))])

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import _ens_truth as ET
        X, Y, ls = ET.problem("q")
        var, _, noise = ET.members("q")
        return dict(X=X, Y=Y, ls=ls, Xs=ET.table("q", 130), variance=float(var[0]), noise=float(noise[0]))

    def exponent_sets(self):
        return [exponents(2, u) for u in UNIFORM]

    def result_exponents(self, k):
        return k

    def device(self, h, p):
        h.set_data(p["X"], p["Y"])
        h.set_params(_kernel_id("rbf"), 0, p["variance"], p["ls"], p["noise"])
        h.set_candidates(p["Xs"])
        lml, logdet, jit = h.fit()
        assert jit == 0.0
        d = collections.OrderedDict([("lml", np.array(lml)), ("logdet", np.array(logdet)), ("alpha", h.alpha())])
        d["mean"], d["var"] = h.predict(True)
        d["dmdx"], d["dvdx"] = h.predict_grad()
        return d


RESIDUE = ResiduePath()


# The parameters through which a Handle method (or a pack's) is handed coordinates, lengthscales or what is tied to them; ``lp`` and
# ``pack`` carry them inside.  tests/test_domains_host.py builds the list of such methods from the signatures and wants every one
# of them named by a family above -- or here, with the reason why no family runs it.
COORDINATE_PARAMETERS = ("X", "Xs", "Xnew", "Xb", "Xc", "Xw", "Xr", "X1", "X2", "Xq", "Z", "lengthscale", "lengthscales", "ranges", "xmin",
                         "xmax", "A", "omega_unit", "r_x0", "s_x0", "lp", "pack")
NOT_COORDINATES = {("qei_set", "Z"): "base samples: standard normals", ("posterior_samples", "Z"): "standard normals",
                   ("sparse_posterior_samples", "Z"): "standard normals", ("debug_gemm", "A"): "a matrix operand of the GEMM probe"}
NOT_COVERED = {
    "Group.set_gower": "gp_group_set_gower hands is_discrete and ranges unchanged to every replica's gp_set_gower, which the Gower "
                       "family runs; the group's other coordinate-taking entries run in the local-penalisation family",
}
# Every other parameter name the public methods have today.  A new entry whose parameter is in neither list fails
# tests/test_domains_host.py until it has been put into one of them: a coordinate under a new name cannot pass unnoticed.
OTHER_PARAMETERS = frozenset((
    "B", "C", "G", "K", "Mz", "Q", "R", "W", "Y", "Yall", "a", "alpha", "ard", "b", "bounds", "c0", "c1", "c_mean", "c_std", "cap",
    "cell_hi", "cell_lo", "cov", "d", "deg", "device", "devices", "ds", "exclude", "fmin", "grad", "handles", "idx", "idxs",
    "include_noise", "is_discrete", "k", "kernel", "key", "levels", "logP", "max_sweeps", "maxtries", "mean", "mean_only", "median",
    "mode", "mu", "n_terms", "name", "nls", "noise", "noises", "nranks", "nsig", "on", "par", "partials", "path", "phase", "posterior",
    "psi", "psis", "r0", "r1", "rank", "root", "rows", "scale", "sense", "shift", "tol", "transform", "tri", "type_", "u", "uid", "val",
    "vals", "value", "var", "variance", "variances", "w", "want_warped", "warp", "y", "y_mean", "y_std", "ystar", "z", "z_eps"))


def covered_methods():
    return sorted(set(m for f in FAMILIES.values() for m in f.methods))


def table():
    """The case table as text: per family its source, the results held bit for bit, those multiplied back, those left out of part 1
    with their formula, and the offsets of part 2."""
    lines = []
    for f in FAMILIES.values():
        exact = [n for n, k in f.results.items() if k == EXACT or isinstance(k, Index)]
        resc = [n for n, k in f.results.items() if isinstance(k, Grad)]
        out = [(n, k.why) for n, k in f.results.items() if isinstance(k, LeftOut)]
        lines.append("%s\n    source: %s\n    exponents: %s\n    offsets: %s%s" % (f.name, f.source, [[int(v) for v in k[:5]] for k in f.exponent_sets()],
                                                                               [float(v) for v in f.offset()[:4]],
                                                                               ("  (%s)" % f.offset_note) if f.offset_note else ""))
        lines.append("    same bits: %s" % ", ".join(exact))
        lines.append("    same bits after 2^(+-k_d): %s" % (", ".join(resc) or "-"))
        for n, why in out:
            lines.append("    left out of part 1: %s -- %s" % (n, why))
    r = RESIDUE
    lines.append("%s (emulate_fp64 = 1; part 1 alone)\n    source: %s\n    exponents: %s" % (r.name, r.source, [[int(v) for v in k] for k in r.exponent_sets()]))
    lines.append("    same bits: %s" % ", ".join(n for n, k in r.results.items() if k == EXACT))
    lines.append("    same bits after 2^(+-k_d): %s" % ", ".join(n for n, k in r.results.items() if isinstance(k, Grad)))
    return lines


# ---- Delta and the allowance ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shifted_problem(name):
    f = FAMILIES[name]
    return shifted(f.problem(), f.roles, f.offset())


@functools.lru_cache(maxsize=None)
def shifted_truth(name):
    """(truth, existing tolerance, Delta) per result of a family's shifted problem, computed once."""
    f = FAMILIES[name]
    p = shifted_problem(name)
    t = f.truth(p)
    tol = f.tolerance(p, t)
    dl = {n: 0.0 for n in t}
    for ls in f.lengthscales(p):
        for how in ("div", "mul"):
            t2 = f.truth(rounded(p, getattr(f, "round_roles", f.roles), ls, how))
            for n in t:
                if not isinstance(f.results[n], Index):
                    dl[n] = max(dl[n], maxnorm(t[n], t2[n]))
    return t, tol, dl


def condition(name):
    """{result: (2 Delta, 10 x the existing tolerance's largest entry)}: the first must not exceed the second."""
    f = FAMILIES[name]
    t, tol, dl = shifted_truth(name)
    return {n: (2 * dl[n], 10 * float(np.max(tol[n]))) for n in t if not isinstance(f.results[n], Index)}


def part2_report(name, dev):
    """Per result of the shifted problem: (device error, existing tolerance at the worst entry, Delta, error / allowance), the
    last the largest over the entries of  |device - truth| / (existing + 2 Delta).  An arg-best passes where the device's row
    scores within twice the allowance of the truth's best (the tie rule of tests/test_gpu_kernel_families.py)."""
    f = FAMILIES[name]
    t, tol, dl = shifted_truth(name)
    rep = collections.OrderedDict()
    for n, kind in f.results.items():
        if isinstance(kind, Index):                             # one index, or one per row of a [S, M] table
            want, got = np.atleast_1d(t[n]).astype(int), np.atleast_1d(dev[n]).astype(int)
            assert want.shape == got.shape, (n, want.shape, got.shape)
            ref = np.asarray(t[kind.of], dtype=T).reshape(want.size, -1)
            allow = (np.asarray(tol[kind.of], dtype=T) + 2 * T(dl[kind.of])) * np.ones(t[kind.of].shape, dtype=T)
            allow = allow.reshape(want.size, -1)
            rows = np.arange(want.size)
            gap = kind.sense * (ref[rows, want] - ref[rows, got])
            rep[n] = (float(np.max(gap)), float(np.max(tol[kind.of])), dl[kind.of], float(np.max(gap / (2 * allow[rows, got]))))
            continue
        got, ref = np.asarray(dev[n], dtype=T), np.asarray(t[n], dtype=T)
        assert got.shape == ref.shape, (n, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), n
        err = np.abs(got - ref)
        allow = np.asarray(tol[n], dtype=T) + 2 * T(dl[n])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.max(np.where(err == 0, T(0), err / allow)))
        rep[n] = (float(np.max(err)), float(np.max(tol[n])), dl[n], ratio)
    return rep


def format_report(name, rep):
    lines = ["%s" % name]
    for n, (err, tol, dl, ratio) in rep.items():
        lines.append("    %-28s Delta %.3e  existing %.3e  device error %.3e  error / (existing + 2 Delta) %.3e" % (n, dl, tol, err, ratio))
    return lines
