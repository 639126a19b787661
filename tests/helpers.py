"""Shared test helpers: run the oracle and the HIP path on the same seeded inputs."""
import numpy as np


def oracle_sample(O, target, Z0, N, K, G, blocks, eps, gamma, seed, temperature=None, schedule=0, init="last_rows",
                  X0=None, lp0=None, rng_offset=0, threads=0):
    """Oracle twin of demcz_sample's generation loop.  Returns dict(chain, log_obj, X, logp, Z, M, changed).
    threads > 0: the oracle's OpenMP loop over chains (synchronous schedule; the same bits as one thread)."""
    M0, d = Z0.shape
    Mcap = M0 + -(-N * G // K)
    prob = O.Problem(N, d, K, Mcap, eps, seed, blocks=blocks, target=target.spec())
    if X0 is None:
        X = np.array(Z0[M0 - N:], order="F") if init == "last_rows" else np.zeros((N, d), order="F")
    else:
        X = np.array(X0, order="F")
    lp = O.logp(prob, X) if lp0 is None else np.array(lp0, dtype=np.float64)
    Z = np.zeros((Mcap, d), order="F")
    Z[:M0] = Z0
    M, chain, lobj, changed = O.run(prob, X, lp, Z, M0, 1, G, gamma, temperature=temperature, schedule=schedule,
                                     rng_offset=rng_offset, threads=threads)
    return dict(chain=chain, log_obj=lobj, X=X, logp=lp, Z=Z[:M].copy(), M=M, changed=changed, prob=prob)


SPLIT, SPLIT_WAVE = 100, 164       # DEMCZ_LAYOUT_SPLIT, DEMCZ_LAYOUT_SPLIT_WAVE (include/demcz.h)


def auto_split_layout(d, N, K=10):
    """What lanes_per_chain = 0 selects for MvNormal with one full block: one wave per chain for the smallest populations of every
    d in 2..32 (as many chains as a LIVE launch of it holds: 1024 on MI355X; 2048 at d <= 5 with K a multiple of five, where a
    wave runs two chains), the replicated / cooperating consumers otherwise where they are built (d <= 10, d = 20)."""
    if 2 <= d <= 32 and N <= 1024:
        return SPLIT_WAVE
    if 2 <= d <= 5 and N <= 2048 and K % 5 == 0:
        return SPLIT_WAVE
    return SPLIT


def split_built(d):
    """MvNormal, one full block: dimensions with the eight-lane replicated (d <= 10) or sixteen-lane cooperating (d = 20) consumers."""
    return 2 <= d <= 10 or d == 20


# ---- non-finite inputs: a bit-level comparison, a poisoned starting population, the generation loop with a Python log-density ----
STATE_KEYS = ("chain", "log_obj", "X", "logp", "Z")
NAN_POS = 0x7FF8000000000000
NAN_NEG = 0xFFF8000000000000          # x86's default NaN: what inf - inf gives on the host that prepared Zinit


def _bits(u):
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


def bits_differ(a, b):
    """None when a and b are the same doubles bit for bit outside their NaNs and are NaN at the same places; otherwise a
    line saying where they first differ.  Stricter than np.array_equal (which takes -0.0 for 0.0); a NaN's sign and payload
    are not compared (the oracle's own NaNs come out as 0x7ff8... and 0xfff8... depending on x86's operand order)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return f"shapes {a.shape} and {b.shape}"
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        i = tuple(int(v[0]) for v in np.nonzero(na != nb))
        return f"NaN at {i} in only one of them ({a[i]!r}, reference {b[i]!r}); {int(np.count_nonzero(na != nb))} such places"
    ne = (a.view(np.uint64) != b.view(np.uint64)) & ~na
    if ne.any():
        i = tuple(int(v[0]) for v in np.nonzero(ne))
        return f"bits differ at {i}: {a[i]!r} ({a[i].view(np.uint64):#018x}), reference {b[i]!r} ({b[i].view(np.uint64):#018x}); {int(np.count_nonzero(ne))} such places"
    return None


def same_bits(got, ref, keys=STATE_KEYS, what=""):
    """Assert that got[k] and ref[k] are the same doubles in the sense of bits_differ, for every key."""
    for k in keys:
        why = bits_differ(got[k], ref[k])
        assert why is None, f"{what}: {k}: {why}"
    return True


# (1.3e154 squared is finite, 1.4e154 squared overflows.  The library's own sentinel, 0xFFF4DEADC0DE5EED, is reserved: not here.)
POISON_VALUES = (1e200, -1e200, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, -0.0, 1.3e154, 1.4e154, -1.4e154,
                 np.finfo(np.float64).max, _bits(NAN_POS), _bits(NAN_NEG))


def poisoned_population(d, N, seed, chain_offset=5):
    """Zinit of 2N + 40 rows (archive-only rows exist at every N) whose last N rows are the chains: standard normals, with one
    value of POISON_VALUES in one coordinate of a quarter of the archive-only rows and of a quarter of the chain rows, cycling
    through the list (the chains start it at chain_offset)."""
    n_arch = N + 40
    Z = np.array(np.random.default_rng(seed).standard_normal((n_arch + N, d)), order="F")
    bits = Z.view(np.uint64)
    values = np.array(POISON_VALUES, dtype=np.float64).view(np.uint64)
    r = np.random.default_rng([seed, 1])
    for base, n, offset in ((0, n_arch, 0), (n_arch, N, chain_offset)):
        rows = r.choice(n, size=max(1, n // 4), replace=False)
        for i, row in enumerate(rows):
            bits[base + row, r.integers(d)] = values[(i + offset) % len(values)]
    return Z


def py_fma(a, b, c):
    """fma(a, b, c) in one rounding: math.fma where the interpreter has it, else exact rational arithmetic (int / int division is
    correctly rounded in CPython, subnormal results included)."""
    import math
    if hasattr(math, "fma"):
        try:
            return math.fma(a, b, c)
        except (OverflowError, ValueError):      # (math.fma raises where IEEE returns inf / nan)
            pass
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b)):
        return a * b + c
    if not math.isfinite(c):
        return c
    from fractions import Fraction
    s = Fraction(a) * Fraction(b) + Fraction(c)
    if s == 0:
        return a * b + c if (a == 0.0 or b == 0.0) else 0.0      # (an exact cancellation rounds to +0)
    try:
        return float(s)
    except OverflowError:
        return math.inf if s > 0 else -math.inf


def oracle_sample_logobj(O, logobj, Z0, N, K, G, blocks, eps, gamma, seed, temperature=None, X0=None, lp0=None, g_from=1,
                         with_xprop=False, rng_offset=0):
    """The oracle's generation loop (synchronous schedule) around a Python log-density: of every block-step only what does not
    depend on the target is taken from the oracle (O.block_step on a problem with a built-in target: the proposal and log u, the
    draw contract's bits); logobj is evaluated on a list of Python floats, and the accept test log u < (lp' - lp) [/ T] and the
    per-generation count (lp_after - lp_before) != 0 are made in NumPy float64, so that +-inf and NaN behave as IEEE says.
    Returns oracle_sample's dict, and `proposed` (N, G, blocks): the log-density of every proposal, accepted or not.
    X0, lp0, g_from: carry a run on -- Z0 is then the archive as it stands, X0 / lp0 the chains, and the G generations are
    g_from .. g_from + G - 1 (temperature[0] is generation g_from's).
    with_xprop: also `xprop` (N, d, G, blocks): every proposal itself, accepted or not -- all d coordinates, those outside the
    block being the bits of the state the block-step started from.  rng_offset: generations a previous run already drew from
    every chain's stream (oracle_sample's)."""
    Z0 = np.asarray(Z0, dtype=np.float64)
    M0, d = Z0.shape
    Mcap = M0 + -(-N * G // K) + (N if g_from > 1 else 0)
    blocks = [list(range(d))] if blocks is None else [list(b) for b in blocks]
    prob = O.Problem(N, d, K, Mcap, eps, seed, blocks=blocks, target=dict(kind="iso_quad", mu=np.zeros(d)))
    f = lambda x: np.float64(logobj([float(v) for v in x]))
    X = np.array(Z0[M0 - N:] if X0 is None else X0, order="F")
    lp = np.array([f(X[c]) for c in range(N)], dtype=np.float64) if lp0 is None else np.array(lp0, dtype=np.float64)
    Z = np.zeros((Mcap, d), order="F")
    Z[:M0] = Z0
    M = M0
    chain = np.zeros((N, d, G), order="F")
    lobj = np.zeros((N, G), order="F")
    changed = np.zeros(G, dtype=np.int64)
    proposed = np.zeros((N, G, len(blocks)))
    xprop = np.zeros((N, d, G, len(blocks)), order="F") if with_xprop else None
    with np.errstate(all="ignore"):
        for g in range(g_from, g_from + G):
            T = None if temperature is None else np.float64(temperature[g - g_from])
            for c in range(N):
                x, lpc = X[c].copy(), lp[c]
                for ib in range(len(blocks)):
                    s = O.block_step(prob, Z, M, c, g + rng_offset, ib, gamma, x, 0.0)
                    lpp = proposed[c, g - g_from, ib] = f(s["xprop"])
                    if with_xprop:
                        xprop[c, :, g - g_from, ib] = s["xprop"]
                    dlt = lpp - lpc
                    if T is not None:
                        dlt = dlt / T
                    if np.float64(s["logu"]) < dlt:
                        x, lpc = s["xprop"].copy(), lpp
                if (lpc - lp[c]) != 0:
                    changed[g - g_from] += 1
                X[c], lp[c] = x, lpc
            chain[:, :, g - g_from], lobj[:, g - g_from] = X, lp
            if g % K == 0:
                Z[M:M + N] = X
                M += N
    out = dict(chain=chain, log_obj=lobj, X=X, logp=lp, Z=Z[:M].copy(), M=M, changed=changed, prob=prob, proposed=proposed)
    if with_xprop:
        out["xprop"] = xprop
    return out
