"""TEST-ONLY reference of the snooker update ("snooker generations"), written from the spec and not from
the kernel: one step in plain Python floats (every operation rounded on its own, no fma), the words of the Philox blocks, the
logarithm and the built-in log-densities from the CPU oracle (oracle_py.draw_block / draw_rows / dm_log / logp), program targets
through their Python twins (tests/program_texts.py).  A mixed run takes its ordinary stretches from the oracle's generation loop
(tests/oracle_engine.py, or helpers.oracle_sample_logobj around a Python log-density) and makes the snooker generations here.

Also a vectorised NumPy form of the same step with NumPy's own random numbers (snooker_population_step): the moment test of
tests/test_snooker_cases.py runs it as the only move, with the Jacobian exponent as a parameter."""
import math

import numpy as np

from helpers import oracle_sample_logobj
from oracle_engine import OracleEngine

MIN_NORMAL = 2.0 ** -1022
TWO64 = 1 << 64


def u_open(r):
    """((r >> 12) + 0.5) * 2^-52, exact."""
    return (float(r >> 12) + 0.5) * 2.0 ** -52


def anchor_index(r1, M, i1, i2):
    """The third row: j = floor(r1 (M - 2) / 2^64), stepped over the two rows already drawn, the lower one first."""
    j = (r1 * (M - 2)) // TWO64
    lo, hi = min(i1, i2), max(i1, i2)
    if j >= lo:
        j += 1
    if j >= hi:
        j += 1
    return j


def gamma_s(r2, lo, hi):
    """lo + (hi - lo) * u_open(r2): the product rounded, then the sum."""
    prod = (hi - lo) * u_open(r2)
    return lo + prod


def norm_ok(v):
    """A finite positive normal double: the domain of dm_log."""
    return math.isfinite(v) and v >= MIN_NORMAL


def is_snooker_generation(g, rng_offset, every):
    return every > 0 and (g + rng_offset) % every == 0


def snooker_step(O, seed, chain, B, Z, M, x, lp, logobj, gamma, T=None):
    """One snooker step of global chain `chain` whose generation starts at Philox block B, against archive rows Z[:M].
    x: list of d floats, lp: float, logobj: list of floats -> float, gamma: (lo, hi), T: the generation's temperature or None.
    Returns (x_after, lp_after, facts)."""
    d = len(x)
    i1, i2 = O.draw_rows(seed, chain, B, M)
    r1, r2 = O.draw_block(seed, chain, B + 1)
    ia = anchor_index(r1, M, i1, i2)
    gs = gamma_s(r2, float(gamma[0]), float(gamma[1]))
    r1, _ = O.draw_block(seed, chain, B + 2)
    logu = float(O.dm_log(u_open(r1)))
    a = [float(v) for v in Z[ia]]
    z1 = [float(v) for v in Z[i1]]
    z2 = [float(v) for v in Z[i2]]
    e = [x[p] - a[p] for p in range(d)]
    e2 = e[0] * e[0]
    t = (z1[0] - z2[0]) * e[0]
    for p in range(1, d):
        e2 = e2 + e[p] * e[p]
        t = t + (z1[p] - z2[p]) * e[p]
    facts = dict(i1=i1, i2=i2, ia=ia, gamma_s=gs, logu=logu, e2=e2, valid=False, accepted=False, lp=lp, T=T)
    if not norm_ok(e2):                      # (what follows would divide by it; the step rejects whatever it gives)
        return list(x), lp, facts
    c = gs * (t / e2)
    xp = [x[p] + c * e[p] for p in range(d)]
    f = [xp[p] - a[p] for p in range(d)]
    f2 = f[0] * f[0]
    for p in range(1, d):
        f2 = f2 + f[p] * f[p]
    facts.update(f2=f2, xp=list(xp))
    if not norm_ok(f2):
        return list(x), lp, facts
    facts["valid"] = True
    lpp = float(logobj(xp))
    jac = (0.5 * float(d - 1)) * (float(O.dm_log(f2)) - float(O.dm_log(e2)))
    with np.errstate(all="ignore"):
        dlt = np.float64(lpp) - np.float64(lp)
        if T is not None:
            dlt = dlt / np.float64(T)        # (NumPy: T = 0 gives +-inf or NaN as IEEE says, where Python raises)
        accept = bool(np.float64(logu) < dlt + np.float64(jac))
    facts.update(lp_prop=lpp, jac=jac, accepted=accept, dlt=float(dlt))      # dlt: as it entered the comparison, after the division by T
    return (xp, lpp, facts) if accept else (list(x), lp, facts)


class MixedRun:
    """The state of a reference run with snooker generations: run(g_from, g_to) may be called piece by piece, like demcz_run.

    target: a device target with .spec() (the oracle's built-in log-densities), or None with `closure` (a Python log-density on a
    list of floats: the twin of a program target)."""

    def __init__(self, O, *, N, d, K, G, blocks, eps, seed, Z0, target=None, closure=None, every=0, gamma_s=(1.2, 2.2),
                 chain_id0=0, rng_offset=0, external=False, X0=None, lp0=None, extra_rows=0):
        self.O, self.N, self.d, self.K, self.G, self.seed = O, N, d, K, G, seed
        self.blocks = [list(range(d))] if blocks is None else [list(b) for b in blocks]
        self.eps, self.every, self.gamma_s = np.asarray(eps, dtype=np.float64), int(every), gamma_s
        self.chain_id0, self.rng_offset, self.external = chain_id0, rng_offset, external
        self.closure = closure
        Z0 = np.asarray(Z0, dtype=np.float64)
        M0 = Z0.shape[0]
        self.Mcap = M0 + -(-N * G // K) + N + extra_rows
        X = np.array(Z0[M0 - N:] if X0 is None else X0, order="F")
        if closure is None:
            self.eng = OracleEngine(N=N, d=d, K=K, Mcap=self.Mcap, Gcap=G, blockindex=self.blocks, eps_scale=self.eps, seed=seed,
                                    target=target, chain_id0=chain_id0)
            self.eng.set_rng_offset(rng_offset)
            self.eng.set_external_append(external)
            self.eng.set_state(X, lp0, Z0)
            self.S = self.eng.prob.blocks_per_generation()
            prob = self.eng.prob
            self.logobj = lambda xq: float(O.logp(prob, np.array([xq], dtype=np.float64))[0])
        else:
            assert rng_offset == 0 and chain_id0 == 0 and not external, "the Python-log-density loop has no such options"
            self.S = sum(1 + ((1 if len(b) == 1 else len(b)) + 1) // 2 + 1 for b in self.blocks)
            self.logobj = closure
            self.X = X
            self.lp = np.array([np.float64(closure([float(v) for v in X[c]])) for c in range(N)]) if lp0 is None else np.array(lp0, dtype=np.float64)
            self.Z = np.zeros((self.Mcap, d), order="F")
            self.Z[:M0] = Z0
            self.Mrows = M0
            self.chain = np.zeros((N, d, G), order="F")
            self.log_obj = np.zeros((N, G), order="F")
            self.changed = np.zeros(G, dtype=np.int64)
        self.steps = []          # (g, chain, facts) of every snooker step
        self.snooker_generations = []

    # the state, wherever it lives
    def _st(self):
        return self.eng if self.closure is None else self

    @property
    def M(self):
        return self.eng.M if self.closure is None else self.Mrows

    def append_rows(self, rows):
        if self.closure is None:
            self.eng.append_rows(rows)
        else:
            n = rows.shape[0]
            self.Z[self.Mrows:self.Mrows + n] = rows
            self.Mrows += n

    def _ordinary(self, a, b, gamma, temperature):
        if self.closure is None:
            self.eng.run(a, b, gamma, temperature)
            return
        r = oracle_sample_logobj(self.O, self.closure, self.Z[:self.Mrows], self.N, self.K, b - a + 1, self.blocks, self.eps, gamma,
                                 self.seed, temperature=temperature, X0=self.X, lp0=self.lp, g_from=a)
        self.X, self.lp = r["X"], r["logp"]
        self.Z[:r["M"]] = r["Z"]
        self.Mrows = r["M"]
        self.chain[:, :, a - 1:b], self.log_obj[:, a - 1:b], self.changed[a - 1:b] = r["chain"], r["log_obj"], r["changed"]

    def _snooker(self, g, T):
        st = self._st()
        Z, M = st.Z, self.M
        B = (g + self.rng_offset - 1) * self.S
        nch = 0
        for c in range(self.N):
            x = [float(v) for v in st.X[c]]
            lp = float(st.lp[c])
            xn, lpn, facts = snooker_step(self.O, self.seed, self.chain_id0 + c, B, Z, M, x, lp, self.logobj, self.gamma_s, T)
            self.steps.append((g, c, facts))
            with np.errstate(all="ignore"):
                if (np.float64(lpn) - np.float64(lp)) != 0:
                    nch += 1
            st.X[c] = xn
            st.lp[c] = lpn
        st.chain[:, :, g - 1] = st.X
        st.log_obj[:, g - 1] = st.lp
        st.changed[g - 1] = nch
        self.snooker_generations.append(g)
        if g % self.K == 0 and not self.external:
            self.append_rows(st.X.copy())

    def run(self, g_from, g_to, gamma, temperature=None):
        """Generations g_from..g_to; temperature: one per generation of this call, or None."""
        temperature = None if temperature is None else np.asarray(temperature, dtype=np.float64)
        g = g_from
        while g <= g_to:
            if is_snooker_generation(g, self.rng_offset, self.every):
                self._snooker(g, None if temperature is None else float(temperature[g - g_from]))
                g += 1
                continue
            e = g
            while e + 1 <= g_to and not is_snooker_generation(e + 1, self.rng_offset, self.every):
                e += 1
            self._ordinary(g, e, gamma, None if temperature is None else temperature[g - g_from:e - g_from + 1])
            g = e + 1

    def result(self):
        st = self._st()
        return dict(chain=st.chain.copy(order="F"), log_obj=st.log_obj.copy(order="F"), X=st.X.copy(order="F"), logp=np.array(st.lp),
                    Z=st.Z[:self.M].copy(order="F"), M=self.M, changed=st.changed.copy())


# ---- the same step for a whole population in NumPy, with NumPy's random numbers (statistics, not bits) ---------------------------------
def snooker_population_step(rng, X, lp, Z, logp, gamma=(1.2, 2.2), jac_power=None):
    """X (N, d), lp (N,), Z (M, d) -> the population after one snooker step of every chain.  jac_power: the exponent of
    |x' - a| / |x - a| in the accept test; None: the spec's d - 1.  -inf: no Jacobian at all."""
    N, d = X.shape
    M = Z.shape[0]
    i1 = rng.integers(0, M, N)
    i2 = rng.integers(0, M - 1, N)
    i2 = i2 + (i2 >= i1)
    lo, hi = np.minimum(i1, i2), np.maximum(i1, i2)
    ia = rng.integers(0, M - 2, N)
    ia = ia + (ia >= lo)
    ia = ia + (ia >= hi)
    gs = gamma[0] + (gamma[1] - gamma[0]) * rng.random(N)
    logu = np.log(rng.random(N))
    a = Z[ia]
    e = X - a
    e2 = (e * e).sum(axis=1)
    t = ((Z[i1] - Z[i2]) * e).sum(axis=1)
    with np.errstate(all="ignore"):
        c = gs * (t / e2)
        Xp = X + c[:, None] * e
        f = Xp - a
        f2 = (f * f).sum(axis=1)
        valid = np.isfinite(e2) & (e2 >= MIN_NORMAL) & np.isfinite(f2) & (f2 >= MIN_NORMAL)
        lpp = logp(Xp)
        power = (d - 1) if jac_power is None else jac_power
        jac = 0.0 if power == -math.inf else 0.5 * power * (np.log(f2) - np.log(e2))
        acc = valid & (logu < (lpp - lp) + jac)
    Xn = np.where(acc[:, None], Xp, X)
    return Xn, np.where(acc, lpp, lp)
