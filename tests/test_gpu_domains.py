"""GPU: every entry family that reads coordinates, off the unit cube (tests/_domain_cases.py holds the relations, the transforms,
the case table and the reasons).

1. ``test_power_of_two_scales_keep_the_bits``: dimension d of every coordinate and its lengthscale times 2^k_d, k = (-17, 10, 0,
   -3, 6) cycled (one lengthscale: k = -17 everywhere, then +10).  x_d / l_d is the same double, so values, variances, scores, LML,
   alpha, factors, tables and indices come back with the same bits, and gradients with respect to x_d or l_d times 2^k_d do.  No
   tolerance: a copy of the covariance arithmetic that divides after subtracting on one side only, forms a distance from norms, or
   takes the raw coordinate in a gradient moves bits here.
2. ``test_offsets_against_the_truth``: offsets (1000, -37.5, 0, 12) cycled, no scaling, against the family's long-double truth on
   the shifted arrays as the device is given them.  Allowance: what the entry's own test grants plus 2 Delta, Delta measured on
   the truth (what rounding x_d / l_d once moves); tests/test_domains_host.py holds 2 Delta to ten times the existing tolerance.
   Every figure is printed before it is asserted; tools/domain_errors.py keeps them in profiles/domain_errors.txt.

One handle in true fp64 for the module, no option changed.  Option emulate_fp64 = 1 changes no kernel at the sizes of these
cases (one factorisation panel at N <= 768; the sparse and batched entries are always true fp64), so they are not run with it
again; ``test_power_of_two_scales_keep_the_bits_on_the_residue_path`` runs part 1 at N = 1024 on a handle of its own with the
option set, and counts the residue GEMM's launches to show that the path was taken.
"""
import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib

import _domain_cases as DC

pytestmark = pytest.mark.gpu

NAMES = list(DC.FAMILIES)


def _handle(emulate):
    hd = _lib.Handle(0)
    hd.set_option("emulate_fp64", emulate)
    return hd


@pytest.fixture(scope="module")
def h():
    hd = _handle(0)
    yield hd
    hd.close()


def _scales(h, name):
    f = DC.FAMILIES[name]
    p = f.problem()
    base = f.device(h, p)
    assert set(base) == set(f.results), sorted(set(base) ^ set(f.results))
    for v in base.values():
        assert np.all(np.isfinite(v))
    bad = []
    for k in f.exponent_sets():
        moved = f.device(h, DC.scaled(p, f.roles, k))
        fails = DC.part1_failures(f.results, base, moved, f.result_exponents(k))
        print("%-44s k = %s: %d of %d results moved %s" % (name, [int(v) for v in k[:5]], len(fails), len(f.results), fails))
        bad += fails
    assert not bad, bad


def _offsets(h, name):
    f = DC.FAMILIES[name]
    dev = f.device(h, DC.shifted_problem(name))
    rep = DC.part2_report(name, dev)
    print("\n".join(DC.format_report("%s, offsets %s" % (name, [float(v) for v in f.offset()[:4]]), rep)))
    bad = [n for n, r in rep.items() if not r[3] <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_power_of_two_scales_keep_the_bits(h, name):
    _scales(h, name)


@pytest.mark.parametrize("name", NAMES)
def test_offsets_against_the_truth(h, name):
    _offsets(h, name)


def test_power_of_two_scales_keep_the_bits_on_the_residue_path():
    """Part 1 with the trailing update and the candidate solve on the int8 matrix cores (tests/_domain_cases.ResiduePath: 1024
    rows, two panels).  gp_profile(1) only puts events around the launches, so that gp_rns_stats can count them: the residue GEMM
    must have run, equally often on the original and on every scaled problem."""
    f = DC.RESIDUE
    hd = _handle(1)
    try:
        hd.profile(1)
        p = f.problem()
        n0 = hd.rns_stats()["launches"]
        base = f.device(hd, p)
        n1 = hd.rns_stats()["launches"]
        phases = [q["name"] for q in hd.phases()]
        print("residue GEMM launches on the original problem: %d; phases of the last call: %s" % (n1 - n0, phases))
        first = n1 - n0
        assert first > 0
        assert set(base) == set(f.results)
        bad = []
        for k in f.exponent_sets():
            moved = f.device(hd, DC.scaled(p, f.roles, k))
            n2 = hd.rns_stats()["launches"]
            fails = DC.part1_failures(f.results, base, moved, f.result_exponents(k))
            print("%-44s k = %s: %d of %d results moved %s (%d residue launches)" % (f.name, [int(v) for v in k], len(fails), len(f.results), fails, n2 - n1))
            assert n2 - n1 == first
            n1 = n2
            bad += fails
        assert not bad, bad
    finally:
        hd.profile(0)
        hd.close()
