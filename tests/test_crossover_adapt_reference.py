"""CPU: the pieces of tests/crossover_adapt_reference.py ("adaptation of the class weights"): the order of the
sums behind rsd, the quantisation of a step's jump distance, the weight rule at its edges, the overflow bound."""
import math

import numpy as np
import pytest

import crossover_adapt_reference as ar


def _ulp(x):
    return math.ulp(abs(x))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 100, 130, 200])
def test_column_sum_is_the_exact_sum_to_a_few_ulp(n):
    r = np.random.default_rng(n)
    v = [float(x) for x in r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)]
    exact = math.fsum(v)
    scale = math.fsum(abs(x) for x in v)
    # n - 1 additions in a tree of depth <= ceil(n / 64) + 6, each with a relative error of 2^-53 of a partial sum <= scale
    assert abs(ar.column_sum(v) - exact) <= (-(-n // 64) + 6) * _ulp(scale)


def test_the_order_of_the_sum_is_pinned():
    """A column where the order changes the last bit: lane 0 adds chains 0 and 64 first, then the butterfly adds lane 32's."""
    v = [0.0] * 100
    v[0], v[64], v[32] = 1.0, 2.0 ** -53, 2.0 ** -53
    # lane 0: 1 + 2^-53 = 1 (ties to even); + lane 32's 2^-53 = 1 again.  In chain order 0, 32, 64 the result is the same 1.0; with
    # the two small ones added first (2^-52) it is 1 + 2^-52
    assert ar.column_sum(v) == 1.0
    assert (v[32] + v[64]) + v[0] == 1.0 + 2.0 ** -52
    # and the other way round: the lanes of the upper half are added to each other before they reach lane 0
    w = [0.0] * 64
    w[0], w[16], w[48] = 1.0, 2.0 ** -53, 2.0 ** -53
    # s = 32: lane 16 += lane 48 -> 2^-52; s = 16: lane 0 += lane 16 -> 1 + 2^-52; sequentially it would stay 1.0
    assert ar.column_sum(w) == 1.0 + 2.0 ** -52
    assert (w[0] + w[16]) + w[48] == 1.0


@pytest.mark.parametrize("n", [2, 64, 70, 100])
def test_rsd_is_the_reciprocal_standard_deviation(n):
    r = np.random.default_rng(100 + n)
    x = 3.0 + 2.0 * r.standard_normal(n)
    want = 1.0 / math.sqrt(math.fsum((v - math.fsum(x) / n) ** 2 for v in x) / (n - 1))
    assert abs(ar.rsd_of(x) - want) <= 16 * _ulp(want)


def test_rsd_of_what_has_no_spread_is_zero():
    assert ar.rsd_of([0.25] * 100) == 0.0
    assert ar.rsd_of([7.0]) == 0.0                          # N = 1: 0 / 0
    assert ar.rsd_of([1.0, math.inf, 2.0]) == 0.0
    assert ar.rsd_of([1.0, math.nan, 2.0]) == 0.0
    assert ar.rsd_of([1e200, -1e200, 3.0]) == 0.0           # the variance overflows
    assert ar.rsd_all(np.array([[1.0, 5.0], [2.0, 5.0], [4.0, 5.0]]))[1] == 0.0


def test_the_quantum_of_a_step():
    assert ar.quantise(0.0) == 0
    assert ar.quantise(math.nextafter(2.0 ** -16, 0.0)) == 0        # just below one quantum
    assert ar.quantise(2.0 ** -16) == 1
    assert ar.quantise(1.0) == 65536
    assert ar.quantise(1.5 + 2.0 ** -17) == 98304                   # truncating
    assert ar.quantise(math.nextafter(65536.0, 0.0)) == 2 ** 32 - 1
    assert ar.quantise(65536.0) == 2 ** 32
    assert ar.quantise(1e300) == 2 ** 32 and ar.quantise(math.inf) == 2 ** 32
    assert ar.quantise(math.nan) == 0 and ar.quantise(-1.0) == 0 and ar.quantise(-0.0) == 0


def test_the_jump_is_summed_in_parameter_order_and_skips_what_did_not_move():
    x, xp, rsd = [1.0, 2.0, 3.0], [1.5, 2.0, 1.0], [2.0, 5.0, 0.0]
    assert ar.jump(x, xp, rsd) == 1.0                               # (0.5 * 2)^2; the unselected parameter and the rsd = 0 column give 0
    assert math.isnan(ar.jump([math.inf, 0.0], [math.inf, 1.0], [1.0, 1.0])) and ar.quantise(math.nan) == 0


def test_the_weight_rule_at_its_edges():
    w0 = [3, 4, 5]
    assert ar.new_weights(w0, [0, 0, 0], [10, 10, 10], 656) == w0            # R = 0: the weights stay
    assert ar.new_weights(w0, [0, 0, 0], [0, 0, 0], 656) == w0
    # a class never tried has r = 0 and gets the floor
    assert ar.new_weights(w0, [100, 300, 999], [1, 1, 0], 656) == [16384, 49152, 656]
    # the floor, and truncation: r = (1, 2) / 3 -> 21845.33 and 43690.67
    assert ar.new_weights([1, 1], [1, 2], [1, 1], 1) == [21845, 43690]
    assert ar.new_weights([1, 1, 1], [1, 1000, 1000], [1, 1, 1], 656) == [656, 32751, 32751]
    assert ar.new_weights([1, 1], [5, 0], [1, 1], 8192) == [65536, 8192]
    # W stays inside [1, 2^31): at most 8 (65536 + 8192)
    assert sum(ar.new_weights([1] * 8, [1] * 8, [1] * 8, 8192)) == 8 * 8192


def test_the_overflow_bound():
    assert ar.fits(100, (2 ** 31 - 1) // 100) and not ar.fits(100, (2 ** 31 - 1) // 100 + 1)
    assert ar.fits(1, 2 ** 31 - 1) and not ar.fits(1, 2 ** 31)
    # the bound is what keeps a class's sum inside 64 bits: every step of every chain at the clamp
    assert (2 ** 31 - 1) * 2 ** 32 < 2 ** 64
