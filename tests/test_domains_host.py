"""CPU: what tests/test_gpu_domains.py rests on (tests/_domain_cases.py), before any device is asked.

1. The long-double truths themselves obey relation 1: on a problem whose coordinates and lengthscales are scaled by 2^k_d they
   return the same numbers, gradients times 2^k_d -- to a few long-double eps (in fact to the bit: a power of two moves no
   mantissa).  This proves the relation per family, and that the transform moves everything that has to move.
2. For every case 2 Delta is at most ten times the entry's existing tolerance, so the allowance of part 2 cannot swallow a real
   error; a case that needs a smaller first offset than 1000 says so in the table.
3. The table names every ``Handle``, pack and ``Group`` method that is handed coordinates, lengthscales or what is tied to them:
   the list is built from the signatures, and every parameter name of every public method must be classified, so a new entry
   without a row fails here whatever it calls its arguments.
4. The transforms do what they say (exact scaling, the inverse for slopes, one exponent for radii), and the comparison of part 1
   rejects a moved bit.
"""
import inspect

import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib

import _domain_cases as DC

NAMES = list(DC.FAMILIES)
FEW_EPS = 4.0


@pytest.mark.parametrize("name", NAMES)
def test_the_truth_obeys_relation_1(name):
    f = DC.FAMILIES[name]
    p = f.problem()
    base = f.truth(p)
    assert set(base) == set(f.results), sorted(set(base) ^ set(f.results))
    for k in f.exponent_sets():
        moved = f.truth(DC.scaled(p, f.roles, k))
        gap = DC.part1_truth_gap(f.results, base, moved, f.result_exponents(k))
        worst = max(gap, key=gap.get)
        print("%-44s k = %s: worst %.2f long-double eps (%s)" % (name, [int(v) for v in k[:5]], gap[worst], worst))
        assert gap[worst] <= FEW_EPS, (worst, gap[worst])
        for n, kind in f.results.items():
            if isinstance(kind, DC.Index):
                assert np.array_equal(base[n], moved[n]), n


@pytest.mark.parametrize("name", NAMES)
def test_two_delta_stays_within_ten_tolerances(name):
    f = DC.FAMILIES[name]
    cond = DC.condition(name)
    for n, (two_delta, ten_tol) in cond.items():
        print("%-44s %-24s 2 Delta %.3e   10 x existing %.3e" % (name, n, two_delta, ten_tol))
    bad = {n: v for n, v in cond.items() if not v[0] <= v[1]}
    assert not bad, bad
    assert (f.first_offset == DC.OFFSETS[0]) == (not f.offset_note)       # a smaller first offset is said in the table


CLASSES = (_lib.Handle, _lib.FeasPack, _lib.EhviPack, _lib.Group)


def _public(cls):
    for name, fn in inspect.getmembers(cls, callable):
        if not name.startswith("_") or name == "__init__":
            yield (name if cls is _lib.Handle else "%s.%s" % (cls.__name__, name)), name, fn


def _methods_with_coordinates():
    out = []
    for cls in CLASSES:
        for full, name, fn in _public(cls):
            params = [q for q in inspect.signature(fn).parameters if q in DC.COORDINATE_PARAMETERS and (name, q) not in DC.NOT_COORDINATES]
            if params and name != "__init__":
                out.append(full)
    return sorted(out)


def test_every_parameter_of_every_public_method_is_classified():
    """A coordinate under a new parameter name cannot pass unnoticed: every parameter is a coordinate's or a known other one."""
    unknown = sorted(set("%s(%s)" % (full, q) for cls in CLASSES for full, _, fn in _public(cls) for q in inspect.signature(fn).parameters
                         if q != "self" and q not in DC.COORDINATE_PARAMETERS and q not in DC.OTHER_PARAMETERS))
    assert not unknown, unknown
    assert not set(DC.COORDINATE_PARAMETERS) & DC.OTHER_PARAMETERS


def test_the_table_names_every_method_that_takes_coordinates():
    found = _methods_with_coordinates()
    print(found)
    assert len(found) > 45 and "set_data" in found and "sparse_acq_rows" in found and "FeasPack.rows" in found and "Group.set_data" in found
    covered = set(DC.covered_methods())
    missing = [m for m in found if m not in covered and m not in DC.NOT_COVERED]
    assert not missing, missing
    assert not [m for m in DC.NOT_COVERED if m in covered]
    assert list(DC.NOT_COVERED) == ["Group.set_gower"]
    for m in covered | set(DC.NOT_COVERED):        # and nothing in the table is a method that does not exist
        cls, _, name = m.rpartition(".")
        assert hasattr(getattr(_lib, cls) if cls else _lib.Handle, name), m


def test_the_table_has_a_row_per_family_and_quotes_what_it_leaves_out():
    text = "\n".join(DC.table())
    for fam in ("dense anchor", "local penalisation", "mean function", "append", "cost", "feasibility", "MES", "paths", "qEI", "EHVI",
                "entropy search", "sparse", "ensemble", "input warping", "Gower"):
        assert any(n.startswith(fam) for n in NAMES), fam
    assert {f.ard for f in DC.FAMILIES.values()} == {True, False}
    out = [(f.name, n) for f in DC.FAMILIES.values() for n, k in f.results.items() if isinstance(k, DC.LeftOut)]
    assert out == [("local penalisation", "dlp"), ("local penalisation", "rows6 dlp")]       # one formula, nothing else
    assert "phi(z_b) / (Phi(z_b) s_b |x - Xb_b|)" in text


def test_transforms():
    rng = np.random.default_rng(0)
    p = dict(X=rng.uniform(0, 1, (7, 5)), sets=(rng.uniform(0, 1, (3, 5)), rng.uniform(0, 1, (2, 5))), ls=rng.uniform(0.5, 1, 5),
             A=rng.standard_normal((5, 2)), r=np.array([0.1, 0.2]), other=np.arange(3.0))
    roles = dict(X=DC.COORD, sets=DC.COORD, ls=DC.LENGTH, A=DC.SLOPE)
    k = DC.exponents(5)
    assert list(k) == [-17, 10, 0, -3, 6] and list(DC.exponents(7)[5:]) == [-17, 10]
    q = DC.scaled(p, roles, k)
    assert np.array_equal(q["X"] / q["ls"], p["X"] / p["ls"]) and np.array_equal(q["sets"][1] / q["ls"], p["sets"][1] / p["ls"])
    assert np.array_equal(q["X"][:, :, None] * q["A"][None], p["X"][:, :, None] * p["A"][None])      # the products x_d A_d do not move
    assert q["other"] is p["other"] and np.array_equal(q["X"], p["X"] * 2.0 ** k)
    with pytest.raises(AssertionError):
        DC.scaled(p, dict(r=DC.RADIUS), k)                                          # a radius takes one exponent
    assert np.array_equal(DC.scaled(p, dict(r=DC.RADIUS), DC.exponents(5, 10))["r"], p["r"] * 1024.0)
    assert list(DC.offsets(5)) == [1000.0, -37.5, 0.0, 12.0, 1000.0] and list(DC.offsets(2, 250.0)) == [250.0, -37.5]
    s = DC.shifted(p, roles, DC.offsets(5))
    assert np.array_equal(s["X"], p["X"] + DC.offsets(5)) and s["ls"] is p["ls"] and s["A"] is p["A"]
    masked = DC.scaled(p, dict(X=DC.only(DC.COORD, (1,), 5)), k)
    assert np.array_equal(masked["X"][:, 1], p["X"][:, 1] * 1024.0) and np.array_equal(masked["X"][:, 0], p["X"][:, 0])
    for how in ("div", "mul"):
        r = DC.rounded(s, roles, p["ls"], how)["X"]
        assert r.dtype == np.longdouble
        rel = np.max(np.abs(r - s["X"]) / np.abs(np.where(s["X"] == 0, 1, s["X"])))
        assert 0 < rel <= (2.0 if how == "div" else 3.0) * 2.0 ** -53               # one rounding of x / l (two with the reciprocal)


def test_part_1_rejects_a_moved_bit():
    results = {"v": DC.EXACT, "g": DC.grad(1), "i": DC.Index("v", -1)}
    k = np.array([-17, 10, 0])
    base = {"v": np.array([1.0, 2.0]), "g": np.ones((2, 3)), "i": np.array(1)}
    moved = {"v": base["v"].copy(), "g": base["g"] * 2.0 ** -k, "i": np.array(1)}
    assert DC.part1_failures(results, base, moved, k) == []
    moved["v"][1] = np.nextafter(2.0, 3.0)
    moved["g"][0, 0] = np.nextafter(moved["g"][0, 0], 0.0)
    moved["i"] = np.array(0)
    assert [b.split(" ")[0] for b in DC.part1_failures(results, base, moved, k)] == ["v", "g", "i"]
    assert not DC.same_bits(np.array([0.0]), np.array([-0.0]))
