"""TEST-ONLY reference of the adaptation of the crossover class weights ("adaptation of the class weights"),
written from the specification alone: plain Python integers and floats, every operation rounded on its own.

AdaptRun is crossover_reference.CrossoverRun with the adaptation's state beside it: per class the weights, the quantised jump
distance and the steps tried; the reciprocal standard deviations of the parameters over the chains; the updates made.  The steps
themselves are CrossoverRun's -- this class only changes the cumulative weights they draw their class with, at the update
positions.  state() is what demcz_get_crossover_adapt answers."""
import math

import numpy as np

import crossover_reference as cr

LANES = 64
Q_ONE = 65536.0          # a jump distance of 1 in the quantised sum, and the clamp of one step's J
W_ONE = 65536.0          # the weights of one update sum to about this


def column_sum(vals):
    """The sum of one column over the chains in THE order: lane l adds the chains c = l, l + 64, ... in increasing c onto 0.0; then
    a_l = a_l + a_(l + s) for s = 32 ... 1 (all lanes at once: lane l < s reads a lane >= s, which this step does not write)."""
    a = [0.0] * LANES
    for c, v in enumerate(vals):
        a[c % LANES] = a[c % LANES] + v
    s = LANES // 2
    while s >= 1:
        for lane in range(s):
            a[lane] = a[lane] + a[lane + s]
        s //= 2
    return a[0]


def rsd_of(column):
    """1 / sd of a column, two passes; 0.0 where the variance is not a positive finite number (a constant column, N = 1, inf, NaN)"""
    x = [float(v) for v in column]
    n = len(x)
    mean = column_sum(x) / float(n)
    sq = []
    for v in x:
        t = v - mean
        sq.append(t * t)
    ss = column_sum(sq)
    with np.errstate(all="ignore"):
        var = float(np.float64(ss) / np.float64(float(n - 1)))      # (0 / 0 with one chain)
    if var > 0.0 and var < math.inf:
        return 1.0 / math.sqrt(var)
    return 0.0


def rsd_all(X):
    return [rsd_of(X[:, p]) for p in range(X.shape[1])]


def jump(x, xp, rsd):
    """J = sum_p ((x'_p - x_p) rsd_p)^2 in increasing p from 0.0"""
    J = 0.0
    for p in range(len(x)):
        t = (float(xp[p]) - float(x[p])) * rsd[p]
        J = J + t * t
    return J


def quantise(J):
    """(J >= 0) ? (uint64)(min(J, 65536) * 65536) : 0, truncating; NaN gives 0"""
    if not J >= 0.0:
        return 0
    return int((J if J < Q_ONE else Q_ONE) * Q_ONE)


def new_weights(weights, dist, tried, min_weight):
    """The update rule: the weights stay where nothing has been measured yet (R = 0)."""
    r = [float(dist[k]) / float(tried[k]) if tried[k] > 0 else 0.0 for k in range(len(weights))]
    R = 0.0
    for v in r:
        R = R + v
    if not R > 0.0:
        return list(weights)
    return [max(int(min_weight), int(v / R * W_ONE)) for v in r]


def fits(N, until):
    """a step adds at most 2^32 to a 64-bit sum: N * until < 2^31"""
    return N * until < (1 << 31)


class AdaptRun(cr.CrossoverRun):
    """CrossoverRun with adapted class weights.  adapt_every / adapt_until / min_weight: demcz_set_crossover_adapt's; adapt_state:
    a state() to continue from (the spread is then not computed at the start)."""

    def __init__(self, O, *, adapt_every, adapt_until, min_weight=656, adapt_state=None, **kw):
        super().__init__(O, **kw)
        assert adapt_every >= 1 and adapt_until >= adapt_every and adapt_until % adapt_every == 0 and 1 <= min_weight <= 8192
        assert fits(self.N, adapt_until)
        self.adapt_every, self.adapt_until, self.min_weight = int(adapt_every), int(adapt_until), int(min_weight)
        if adapt_state is None:
            self.dist, self.tried, self.updates = [0] * self.ncr, [0] * self.ncr, 0
            self.rsd = rsd_all(self.X)
        else:
            self.weights = [int(v) for v in adapt_state["weights"]]
            self.cum = cr.cumulative(self.weights)
            self.dist, self.tried = [int(v) for v in adapt_state["dist"]], [int(v) for v in adapt_state["tried"]]
            self.rsd, self.updates = [float(v) for v in adapt_state["rsd"]], int(adapt_state["updates"])
        self.update_log = []         # (g, weights before, weights after, rsd in force during the period that ended)
        self.jumps = []              # (g, chain, class, J, q) of every accepted step that was accumulated
        self.weights_at = {}         # g -> the weights generation g drew its classes with

    def set_weights(self, weights):
        """demcz_set_crossover_weights"""
        self.weights = [int(v) for v in weights]
        self.cum = cr.cumulative(self.weights)

    def _generation(self, g, gamma, T):
        pos = g + self.rng_offset
        accumulate = pos <= self.adapt_until
        n0 = len(self.steps)
        before = self.X.copy()
        self.weights_at[g] = list(self.weights)
        super()._generation(g, gamma, T)
        if not accumulate:
            return
        for _, c, f in self.steps[n0:]:          # (none in a snooker generation)
            self.tried[f["m"]] += 1
            if f["accepted"]:
                J = jump(before[c], f["xp"], self.rsd)
                q = quantise(J)
                self.dist[f["m"]] += q
                self.jumps.append((g, c, f["m"], J, q))
        if pos % self.adapt_every == 0:
            old, old_rsd = list(self.weights), list(self.rsd)
            self.set_weights(new_weights(self.weights, self.dist, self.tried, self.min_weight))
            self.updates += 1
            self.rsd = rsd_all(self.X)
            self.update_log.append((g, old, list(self.weights), old_rsd))

    def state(self):
        return dict(weights=list(self.weights), dist=list(self.dist), tried=list(self.tried), rsd=list(self.rsd), updates=self.updates)
