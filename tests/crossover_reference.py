"""TEST-ONLY reference of the crossover generation ("crossover generations"), written from the spec and not
from the kernel: one step in plain Python integers and floats (every operation rounded on its own, no fma), the words of the
Philox blocks, the rows, the normals, the logarithm and the built-in log-densities from the CPU oracle (oracle_py.draw_block /
draw_rows / normal_pair / dm_log / logp), program targets through their Python twins (tests/program_texts.py).

CrossoverRun has the interface of snooker_reference.MixedRun (piecewise run, appends at K, external, chain_id0, rng_offset,
temperatures); it makes its snooker generations through snooker_reference.snooker_step, at the crossover stride.  It records the
facts of every step: class, delta, mask, whether the fallback was taken, whether the step was accepted.

Also a vectorised NumPy form of the same proposal with NumPy's own generator (crossover_population_step), for statistics."""
import numpy as np

import snooker_reference as sr

TWO32 = 1 << 32
TWO64 = 1 << 64


def stride(d, delta_max):
    """S_cr: the choices, delta_max pairs, ceil(d / 4) blocks of subset words, ceil(d / 2) of normals, log u."""
    return 1 + delta_max + -(-d // 4) + -(-d // 2) + 1


def words(r1, r2):
    """lo32(r1), hi32(r1), lo32(r2), hi32(r2)"""
    return (r1 & (TWO32 - 1), r1 >> 32, r2 & (TWO32 - 1), r2 >> 32)


def cumulative(weights):
    out, s = [], 0
    for w in weights:
        s += int(w)
        out.append(s)
    return out


def cr_class(word, cum):
    """j = (word W) >> 32; the smallest k with j < w_0 + ... + w_k"""
    j = (word * cum[-1]) >> 32
    for k, c in enumerate(cum):
        if j < c:
            return k
    raise AssertionError("j < W always")


def n_pairs(word, delta_max):
    return 1 + ((word * delta_max) >> 32)


def fallback_parameter(r2, d):
    return (r2 * d) // TWO64


def selects(word, ncr, m):
    """probability (m + 1) / ncr exactly"""
    return word * ncr < ((m + 1) << 32)


def subset(O, seed, chain, B0, d, ncr, m):
    """The selected parameters from the ceil(d / 4) blocks that start at B0: parameter p owns word p mod 4 of block p div 4."""
    sel = []
    for q in range(-(-d // 4)):
        w = words(*O.draw_block(seed, chain, B0 + q))
        for t in range(4):
            p = 4 * q + t
            if p < d and selects(w[t], ncr, m):
                sel.append(p)
    return sel


def proposal(x, sel, diffs, z, gamma, eps):
    """x'_p = x_p + (scale s_p + eps_p z_p) for selected p, x_p itself otherwise; diffs: delta pairs of rows (za, zb);
    scale = gamma / sqrt(2 delta d') with no b == 1 quirk"""
    delta, dsel = len(diffs), len(sel)
    scale = float(np.float64(gamma) / np.sqrt(np.float64(float(2 * delta * dsel))))
    xp = list(x)
    with np.errstate(all="ignore"):
        for p in sel:
            s = np.float64(diffs[0][0][p]) - np.float64(diffs[0][1][p])
            for za, zb in diffs[1:]:
                s = s + (np.float64(za[p]) - np.float64(zb[p]))
            t1 = np.float64(scale) * s
            t2 = np.float64(eps[p]) * np.float64(z[p])
            xp[p] = float(np.float64(x[p]) + (t1 + t2))
    return xp, scale


def crossover_step(O, seed, chain, B, Z, M, x, lp, logobj, gamma, eps, ncr, delta_max, cum, T=None):
    """One crossover step of global chain `chain` whose generation starts at Philox block B, against archive rows Z[:M].
    x: list of d floats, lp: float, logobj: list of floats -> float.  Returns (x_after, lp_after, facts)."""
    d = len(x)
    r1, r2 = O.draw_block(seed, chain, B)
    w = words(r1, r2)
    m = cr_class(w[1], cum)
    delta = n_pairs(w[0], delta_max)
    pstar = fallback_parameter(r2, d)
    pairs = [O.draw_rows(seed, chain, B + 1 + j, M) for j in range(delta_max)]
    B_sub = B + 1 + delta_max
    sel = subset(O, seed, chain, B_sub, d, ncr, m)
    fallback = not sel
    if fallback:
        sel = [pstar]
    B_nrm = B_sub + -(-d // 4)
    z = []
    for pr in range(-(-d // 2)):
        z.extend(O.normal_pair(*O.draw_block(seed, chain, B_nrm + pr)))
    r1, _ = O.draw_block(seed, chain, B_nrm + -(-d // 2))
    logu = float(O.dm_log(sr.u_open(r1)))
    diffs = [([float(v) for v in Z[i1]], [float(v) for v in Z[i2]]) for i1, i2 in pairs[:delta]]
    xp, scale = proposal(x, sel, diffs, z, gamma, eps)
    lpp = float(logobj(xp))
    with np.errstate(all="ignore"):
        dlt = np.float64(lpp) - np.float64(lp)
        raw = bool(np.float64(logu) < dlt)
        if T is not None:
            dlt = dlt / np.float64(T)
        accept = bool(np.float64(logu) < dlt)
    mask = sum(1 << p for p in sel)
    facts = dict(m=m, delta=delta, mask=mask, fallback=fallback, pstar=pstar, pairs=pairs, scale=scale, logu=logu, lp=lp, lp_prop=lpp,
                 accepted=accept, accepted_untempered=raw, T=T, xp=xp)
    return (xp, lpp, facts) if accept else (list(x), lp, facts)


class CrossoverRun:
    """The state of a reference run with crossover (and snooker) generations: run(g_from, g_to) may be called piece by piece.

    target: a device target with .spec() (the oracle's built-in log-densities), or None with `closure` (a Python log-density on a
    list of floats: the twin of a program target)."""

    def __init__(self, O, *, N, d, K, G, eps, seed, Z0, target=None, closure=None, ncr=3, delta_max=3, weights=None, every=0,
                 gamma_s=(1.2, 2.2), chain_id0=0, rng_offset=0, external=False, X0=None, lp0=None, extra_rows=0):
        assert 1 <= ncr <= 8 and 1 <= delta_max <= 3 and d >= 2
        self.O, self.N, self.d, self.K, self.G, self.seed = O, N, d, K, G, seed
        self.eps = [float(v) for v in np.asarray(eps, dtype=np.float64)]
        self.ncr, self.delta_max = ncr, delta_max
        self.weights = [1] * ncr if weights is None else [int(v) for v in weights]
        assert len(self.weights) == ncr and min(self.weights) >= 0 and 1 <= sum(self.weights) < (1 << 31)
        self.cum = cumulative(self.weights)
        self.every, self.gamma_s = int(every), gamma_s
        self.chain_id0, self.rng_offset, self.external = chain_id0, rng_offset, external
        self.S = stride(d, delta_max)
        Z0 = np.asarray(Z0, dtype=np.float64)
        M0 = Z0.shape[0]
        self.Mcap = M0 + -(-N * G // K) + N + extra_rows
        self.X = np.array(Z0[M0 - N:] if X0 is None else X0, order="F")
        if closure is None:
            prob = O.Problem(N, d, K, self.Mcap, np.asarray(eps, dtype=np.float64), seed, blocks=[list(range(d))], chain_id0=chain_id0,
                             target=target.spec())
            self.prob = prob
            self.logobj = lambda xq: float(O.logp(prob, np.array([xq], dtype=np.float64))[0])
        else:
            self.logobj = closure
        self.lp = np.array([np.float64(self.logobj([float(v) for v in self.X[c]])) for c in range(N)]) if lp0 is None else np.array(lp0, dtype=np.float64)
        self.Z = np.zeros((self.Mcap, d), order="F")
        self.Z[:M0] = Z0
        self.M = M0
        self.chain = np.zeros((N, d, G), order="F")
        self.log_obj = np.zeros((N, G), order="F")
        self.changed = np.zeros(G, dtype=np.int64)
        self.steps = []              # (g, chain, facts) of every crossover step
        self.snooker_steps = []      # (g, chain, facts) of every snooker step
        self.snooker_generations = []
        self.crossover_generations = []

    def append_rows(self, rows):
        n = rows.shape[0]
        self.Z[self.M:self.M + n] = rows
        self.M += n

    def _generation(self, g, gamma, T):
        B = (g + self.rng_offset - 1) * self.S
        snooker = sr.is_snooker_generation(g, self.rng_offset, self.every)
        nch = 0
        for c in range(self.N):
            x = [float(v) for v in self.X[c]]
            lp = float(self.lp[c])
            if snooker:
                xn, lpn, facts = sr.snooker_step(self.O, self.seed, self.chain_id0 + c, B, self.Z, self.M, x, lp, self.logobj, self.gamma_s, T)
                self.snooker_steps.append((g, c, facts))
            else:
                xn, lpn, facts = crossover_step(self.O, self.seed, self.chain_id0 + c, B, self.Z, self.M, x, lp, self.logobj, gamma, self.eps,
                                                self.ncr, self.delta_max, self.cum, T)
                self.steps.append((g, c, facts))
            with np.errstate(all="ignore"):
                if (np.float64(lpn) - np.float64(lp)) != 0:
                    nch += 1
            self.X[c] = xn
            self.lp[c] = lpn
        (self.snooker_generations if snooker else self.crossover_generations).append(g)
        self.chain[:, :, g - 1] = self.X
        self.log_obj[:, g - 1] = self.lp
        self.changed[g - 1] = nch
        if g % self.K == 0 and not self.external:
            self.append_rows(self.X.copy())

    def run(self, g_from, g_to, gamma, temperature=None):
        """Generations g_from..g_to; temperature: one per generation of this call, or None."""
        temperature = None if temperature is None else np.asarray(temperature, dtype=np.float64)
        for g in range(g_from, g_to + 1):
            self._generation(g, gamma, None if temperature is None else float(temperature[g - g_from]))

    def counts(self):
        """(tried, accepted) per class over the crossover steps made so far: what demcz_get_crossover answers"""
        tried, acc = np.zeros(self.ncr, dtype=np.int64), np.zeros(self.ncr, dtype=np.int64)
        for _, _, f in self.steps:
            tried[f["m"]] += 1
            acc[f["m"]] += f["accepted"]
        return tried, acc

    def result(self):
        return dict(chain=self.chain.copy(order="F"), log_obj=self.log_obj.copy(order="F"), X=self.X.copy(order="F"), logp=np.array(self.lp),
                    Z=self.Z[:self.M].copy(order="F"), M=self.M, changed=self.changed.copy())


# ---- the same proposal for a whole population in NumPy, with NumPy's own generator (statistics, not bits) -----------------------------
def crossover_population_step(rng, X, lp, Z, logp, gamma, eps, ncr=3, delta_max=3, weights=None):
    """X (N, d), lp (N,), Z (M, d) -> (X, lp, m, accepted) after one crossover step of every chain."""
    N, d = X.shape
    M = Z.shape[0]
    w = np.ones(ncr) if weights is None else np.asarray(weights, dtype=np.float64)
    m = rng.choice(ncr, size=N, p=w / w.sum())
    delta = rng.integers(1, delta_max + 1, N)
    pstar = rng.integers(0, d, N)
    s = np.zeros((N, d))
    for j in range(delta_max):
        i1 = rng.integers(0, M, N)
        i2 = rng.integers(0, M - 1, N)
        i2 = i2 + (i2 >= i1)
        s += np.where((j < delta)[:, None], Z[i1] - Z[i2], 0.0)
    sel = rng.random((N, d)) < ((m + 1) / ncr)[:, None]
    none = ~sel.any(axis=1)
    sel[none, pstar[none]] = True
    dsel = sel.sum(axis=1)
    z = rng.standard_normal((N, d))
    logu = np.log(rng.random(N))
    scale = gamma / np.sqrt(2.0 * delta * dsel)
    Xp = np.where(sel, X + (scale[:, None] * s + eps * z), X)
    lpp = logp(Xp)
    acc = logu < lpp - lp
    return np.where(acc[:, None], Xp, X), np.where(acc, lpp, lp), m, acc
