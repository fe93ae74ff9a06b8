"""The rule of the exact accumulator, pinned where no GPU is needed: a weight x contributes
sign(x) floor(|x| 2^116) units, and is refused iff it is not finite or |x| >= 2^76.  `engine.float_to_limbs`
states it, `tests/limb_cases.units` is the fast form the GPU tests use for every event, and
`limb_cases.kernel_units` is a port of the two shift forms of csrc/hist_device.hpp (`deposit_units`,
`deposit_units_general`) to Python integers with the kernel's word sizes.  All three must agree."""
import math
from fractions import Fraction

import numpy as np

from pisa_amd.engine import float_to_limbs, limbs_to_float
from tests import limb_cases as LC


def _rule(x):
    f = Fraction(float(x)) * (1 << 116)
    return math.floor(f) if f >= 0 else -math.floor(-f)


def _probe_values():
    fam = LC.weight_families()
    vals = [float(v) for k in LC.FAMILY_ORDER for v in fam[k]]
    vals += [float(v) * float(v) for v in vals]                       # the second quantity of the same events
    # every binade from below the format to its top, three mantissas, both signs
    for e in range(-130, 76):
        for m in (1 << 52, LC.M_ONES, LC.M_ALT_A, LC.M_ALT_B):
            vals += [LC.mant(m, e), -LC.mant(m, e)]
    vals += [float(np.nextafter(2.0 ** 76, 0.0)), -float(np.nextafter(2.0 ** 76, 0.0)),
             float(np.nextafter(2.0 ** -52, 0.0)), float(np.nextafter(2.0 ** -52, 1.0)), 2.0 ** -1074, -2.0 ** -1074]
    return vals


def test_families_cover_what_they_claim():
    fam = LC.weight_families()
    assert set(fam) == set(LC.FAMILY_ORDER)
    assert all(LC.kernel_is_fast(w) and LC.kernel_is_fast(w * w) for w in fam["fast_only"].tolist())
    assert not any(LC.kernel_is_fast(w) for w in fam["general_only"].tolist())
    n_fast = sum(LC.kernel_is_fast(w) for w in fam["mixed"].tolist())
    assert 0 < n_fast < len(fam["mixed"])
    assert len(fam["fast_only"]) % 2 == 1 and len(fam["single"]) == 1
    # the leading bit of the mantissa family visits each of the 32 positions of digits 1, 2 and 3
    lead = {LC.kernel_general(w)[0][0] * 32 + int(LC.kernel_general(w)[0][1]).bit_length() - 1
            for w in np.abs(fam["mantissa"]).tolist()}
    assert lead == set(range(32, 128))
    # pairs cancel to the one unit, the copies of 2^37 (1 + 2^-52) to minus one unit
    assert sum(LC.units(w) for w in fam["cancel_pairs"].tolist()) == 1
    assert LC.digits_of(sum(LC.units(w) for w in fam["cancel_pairs"].tolist())) == [1, 0, 0, 0, 0, 0]
    assert LC.digits_of(sum(LC.units(w) for w in fam["cancel_carry_neg"].tolist())) == [0xFFFFFFFF] * 5 + [-1]
    assert all(d != 0 for d in LC.digits_of(sum(LC.units(w) for w in fam["cancel_carry_pos"].tolist()))[:5])


def test_units_float_to_limbs_and_the_kernel_port_state_one_rule():
    vals = _probe_values()
    assert len(vals) > 15000
    for x in vals:
        want = _rule(x)
        assert LC.accepted(x)
        assert LC.units(x) == want, x
        assert LC.limbs_total(float_to_limbs(x)) == want, x
        assert float_to_limbs(x) == LC.digits_of(want), x
        assert LC.kernel_units(x) == want, x
        # the general form alone takes every accepted value as well (the fast form is a special case of it)
        assert sum(v << (32 * j) for j, v in LC.kernel_general(x)) == want, x


def test_the_bottom_of_the_format():
    for x in (5e-324, 2.0 ** -1022, 2.0 ** -117, float(np.nextafter(2.0 ** -116, 0.0)), 0.0, -0.0):
        for s in (1.0, -1.0):
            assert LC.units(s * x) == 0 and LC.kernel_general(s * x) in ([], [(0, 0)]) and float_to_limbs(s * x) == [0] * 6
    assert float_to_limbs(2.0 ** -116) == [1, 0, 0, 0, 0, 0]
    assert LC.units(1.5 * 2.0 ** -116) == 1 and LC.units(-1.5 * 2.0 ** -116) == -1     # truncation towards zero
    assert LC.kernel_units(-1.5 * 2.0 ** -116) == -1
    assert float_to_limbs(-(2.0 ** -116)) == [0xFFFFFFFF] * 5 + [-1]


def test_refusals_are_exactly_the_non_finite_and_the_too_large():
    top = float(np.nextafter(2.0 ** 76, 0.0))
    assert LC.accepted(top) and LC.kernel_units(top) == _rule(top) and LC.kernel_units(-top) == -_rule(top)
    for x in (2.0 ** 76, -2.0 ** 76, float(np.nextafter(2.0 ** 76, np.inf)), 2.0 ** 1023, math.inf, -math.inf, math.nan):
        assert not LC.accepted(x)
        assert LC.kernel_units(x) is None and LC.kernel_general(x) is None and not LC.kernel_is_fast(x)
    # w^2 leaves the range while w is still inside
    assert LC.accepted(2.0 ** 38) and not LC.accepted(2.0 ** 38 * 2.0 ** 38)
    # ... and 2^38 is the first such weight: the square of the double below it rounds DOWN, to 2^76 (1 - 2^-52).  The
    # product of doubles is monotonic, so no weight has a square that rounds up to 2^76 without being >= 2^38 itself.
    below = float(np.nextafter(2.0 ** 38, 0.0))
    assert below * below == 2.0 ** 76 * (1 - 2.0 ** -52) and LC.accepted(below * below)


def test_round_trip_of_values_with_at_most_53_significant_bits():
    rs = np.random.RandomState(2)
    vals = [v for v in _probe_values() if abs(v) >= 2.0 ** -64 or v == 0.0]    # all 53 bits at or above the LSB
    vals += [float(s * LC.mant(int(m) | (1 << 52), int(e)))
             for s, m, e in zip(rs.choice((1.0, -1.0), 500), rs.randint(0, 1 << 52, 500, dtype=np.int64),
                                rs.randint(-64, 76, 500))]
    assert len(vals) > 5000
    for x in vals:
        assert limbs_to_float(float_to_limbs(x)) == x, x
    # the decoder rounds once, to nearest even: 2^53 + 1 units is a tie
    assert limbs_to_float(LC.digits_of((1 << 53) + 1)) == 2.0 ** (53 - 116)
    assert limbs_to_float(LC.digits_of((1 << 53) + 3)) == (2.0 ** 53 + 4) * 2.0 ** -116
    # un-normalised limbs (sums over workgroups and ranks) decode like their canonical form
    assert limbs_to_float([-1, 1, 0, 0, 0, 0]) == LC.value_of((1 << 32) - 1)


def test_exact_sums_and_their_limbs():
    w = np.array([2.0 ** -116, -1.5 * 2.0 ** -116, 3.0, -2.0, 7.0], dtype=np.float64)
    H, S = LC.exact_sums(w, [0, 0, 1, 1, -1], 3)
    assert H == [0, 1 << 116, 0] and S == [0, 13 << 116, 0]
    lim = LC.sums_to_limbs([(H, S)])
    assert lim.shape == (1, 3, 2, 6) and lim[0, 1, 0].tolist() == float_to_limbs(1.0)
    hist, sumw2 = LC.sums_to_maps([(H, S)])
    assert hist.tolist() == [[0.0, 1.0, 0.0]] and sumw2.tolist() == [[0.0, 13.0, 0.0]]
