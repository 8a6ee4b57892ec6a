"""GPU: the knowledge gradient's entries off the unit cube, by the two relations of tests/_domain_cases.py over the cases of
tests/_kg_domain.py (the transforms, exponents and offsets are that module's).

1. Power-of-two scales: dimension d of the data, the discretisation points, the locations and the lengthscale times 2^k_d leaves
   every quotient (x - x') / l the same double: the points' means and both routes' values come back bit for bit, the gradient
   exactly 2^-k_d times the original.
2. Offsets (1000, -37.5, 0, 12, cycled): the device against the long-double truth ON THE SHIFTED ARRAYS, within the existing
   tolerance of tests/test_gpu_kg.py plus 2 Delta (what no double implementation that rounds x_d / l_d once can avoid;
   tests/test_kg_domains_host.py holds 2 Delta to ten times the tolerance)."""
import pytest

from gaussian_process_optimization_amd import _lib

import _domain_cases as DC
import _kg_domain as KD

pytestmark = pytest.mark.gpu


def _handle():
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    return h


@pytest.mark.parametrize("cid", KD.CASES)
def test_power_of_two_scales_change_no_bit(cid):
    p = KD.problem(cid)
    base = KD.device(_handle(), cid, p)
    assert set(base) == set(KD.RESULTS)
    for k in KD.exponent_sets(cid):
        moved = KD.device(_handle(), cid, DC.scaled(p, KD.ROLES, k))
        bad = DC.part1_failures(KD.RESULTS, base, moved, k)
        print("kg case %s  k = %s: %s" % (cid, [int(v) for v in k], "same bits" if not bad else bad))
        assert not bad, bad


@pytest.mark.parametrize("cid", KD.CASES)
def test_offsets_against_the_truth(cid):
    dev = KD.device(_handle(), cid, KD.shifted_problem(cid))
    rep = KD.part2_report(cid, dev)
    for n, (err, tol, dl, ratio) in rep.items():
        print("kg case %s  %-10s Delta %.3e  existing %.3e  device error %.3e  error / (existing + 2 Delta) %.3e" % (cid, n, dl, tol, err, ratio))
    bad = {n: v for n, v in rep.items() if not v[3] <= 1.0}
    assert not bad, bad
