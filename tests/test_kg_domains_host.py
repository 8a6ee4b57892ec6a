"""CPU: what tests/test_domains_host.py asserts for the table of tests/_domain_cases.py, for the knowledge gradient's two cases of
tests/_kg_domain.py: the long-double truth itself obeys the power-of-two relation to a few long-double eps, and 2 Delta stays
within ten times the existing tolerance, so that the offset relation's allowance cannot swallow a real error."""
import numpy as np
import pytest

import _domain_cases as DC
import _kg_domain as KD

FEW_EPS = 4.0      # tests/test_domains_host.py's


@pytest.mark.parametrize("cid", KD.CASES)
def test_the_truth_obeys_the_power_of_two_relation(cid):
    p = KD.problem(cid)
    base = KD.truth(cid, p)
    for k in KD.exponent_sets(cid):
        moved = KD.truth(cid, DC.scaled(p, KD.ROLES, k))
        gap = DC.part1_truth_gap(KD.RESULTS, base, moved, k)
        worst = max(gap, key=gap.get)
        print("kg case %s  k = %s: worst %.2f long-double eps (%s)" % (cid, [int(v) for v in k], gap[worst], worst))
        assert gap[worst] <= FEW_EPS, (worst, gap[worst])


@pytest.mark.parametrize("cid", KD.CASES)
def test_two_delta_stays_within_ten_tolerances(cid):
    cond = KD.condition(cid)
    for n, (two_delta, ten_tol) in cond.items():
        print("kg case %s  %-10s 2 Delta %.3e   10 x existing %.3e" % (cid, n, two_delta, ten_tol))
    bad = {n: v for n, v in cond.items() if not v[0] <= v[1]}
    assert not bad, bad
    assert np.array_equal(KD.offset(cid), DC.offsets(len(KD.offset(cid))))      # that module's offsets, the first one 1000
