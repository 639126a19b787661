"""The reference of bridge sampling (tests/bridge_reference.py) is itself checked here, without a GPU: the fast fma against exact
fractions, the factor and the two sides of the proposal against plain linear algebra, and the whole method against targets whose
marginal likelihood is known -- exact independent draws over 20 seeds each, and one history of the sampler itself run by the
CPU oracle.  The bound of the guards is bridge_reference.GUARD_Z standard errors: twice the largest miss seen, printed below."""
import math

import numpy as np
import pytest

import bridge_reference as br
import bridge_cases as bc
import oracle_py as O

SEEDS = range(20)
N_G, W_G = 32, 200            # the guards' histories: 32 chains x 200 generations, 3200 draws on either side


def test_fast_fma_equals_exact_fractions():
    rng = np.random.default_rng(0)
    n = 4000
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    c = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    # cancellation: c is the rounded product with the other sign, the result is the product's rounding error
    a2, b2 = rng.standard_normal(n), rng.standard_normal(n)
    c2 = -(a2 * b2)
    # ties: products that lie exactly between two doubles once c is added
    a3 = 1.0 + rng.integers(1, 2 ** 20, n) * 2.0 ** -26
    b3 = 1.0 + rng.integers(1, 2 ** 20, n) * 2.0 ** -27
    c3 = rng.integers(1, 2 ** 30, n).astype(np.float64)
    # squares added to a running sum, as the kernels do
    a4 = rng.standard_normal(n)
    c4 = np.abs(rng.standard_normal(n)) * 30.0
    for x, y, z in ((a, b, c), (a2, b2, c2), (a3, b3, c3), (a4, a4, c4), (a, b, np.zeros(n)), (a, np.zeros(n), c)):
        got, want = br.fma_fast(x, y, z), br.fma_exact(x, y, z)
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    # the fall-backs: a product too small for the error-free product, and operands that are not finite
    tiny = np.array([1e-200, 3.0]), np.array([1e-150, 1e-300]), np.array([1e-320, 1e-310])
    assert np.array_equal(br.fma_fast(*tiny), br.fma_exact(*tiny))
    assert br.fma_fast(np.array([np.inf]), np.array([1.0]), np.array([1.0]))[0] == np.inf
    assert np.isnan(br.fma_fast(np.array([np.nan]), np.array([1.0]), np.array([1.0]))[0])


def _random_spd(rng, d):
    A = rng.standard_normal((d, d))
    return A @ A.T / d + 0.5 * np.eye(d)


def test_cholesky_and_its_refusal():
    rng = np.random.default_rng(1)
    worst = 0.0
    for d in (1, 2, 5, 7, 32):
        V = _random_spd(rng, d)
        L = br.cholesky(V)
        assert np.allclose(L, np.linalg.cholesky(V), rtol=1e-12, atol=1e-14) and np.all(np.triu(L, 1) == 0.0)
        worst = max(worst, br.cholesky_error(L, V))
    print(f"[bridge] cholesky: largest |(L L^T - V)_pq| / sqrt(V_pp V_qq) = {worst:.2e} (CHOL_TOL {br.CHOL_TOL:.1e})")
    assert worst <= br.CHOL_TOL / 10.0
    V = _random_spd(rng, 4)
    V[2, :] = V[:, 2] = 0.0                                  # a constant parameter
    with pytest.raises(ValueError, match="parameter 2"):
        br.cholesky(V)


@pytest.mark.parametrize("d", [1, 2, 5, 7])
def test_two_sides_of_the_proposal_agree(d):
    """x = m + L z and the solve L z = x - m are inverse to each other, log g is the normal density, and the draws are the
    oracle's Box-Muller pairs in the order of the spec."""
    rng = np.random.default_rng(10 + d)
    m, L = rng.standard_normal(d), np.linalg.cholesky(_random_spd(rng, d))
    Np, wp, seed = 6, 4, 77
    z = br.proposal_z(seed, Np, wp, d)
    B = (d + 1) // 2
    r1, r2 = O.draw_block(seed, 5, 3 * B + (d - 1) // 2)
    assert z[5, (d - 1) // 2 * 2, 3] == O.normal_pair(r1, r2)[0]
    x, logg = br.proposal(seed, Np, wp, m, L)
    rows = br.rows_of(x)
    assert np.allclose(br.solve_z(rows, m, L), br.rows_of(z), rtol=1e-10, atol=1e-12)
    dev = rows - m
    Vinv = np.linalg.inv(L @ L.T)
    want = -0.5 * np.einsum("ij,jk,ik->i", dev, Vinv, dev) - 0.5 * np.log(np.linalg.det(2.0 * math.pi * (L @ L.T)))
    assert np.allclose(logg.ravel(), want, rtol=1e-10, atol=1e-10)
    lp = rng.standard_normal((Np, wp))
    a1 = br.posterior_a1(x, lp, m, L)
    assert np.allclose(a1, lp - logg, rtol=1e-10, atol=1e-10)


# ---- targets whose marginal likelihood is known ------------------------------------------------------------------------------------
def _phi_upper(a):
    return 0.5 * math.erfc(a / math.sqrt(2.0))


def _gaussian(d, seed):
    """log_obj = 3 - 0.5 sum ((x_p - p) / s_p)^2: log Z = 3 + d/2 log 2 pi + sum log s_p."""
    rng = np.random.default_rng(1000 * d + seed)
    s = 0.5 + np.arange(d) % 3
    mu = np.arange(d, dtype=np.float64)
    logobj = lambda x: 3.0 - 0.5 * (((x - mu) / s) ** 2).sum(axis=1)     # noqa: E731
    draws = mu + s * rng.standard_normal((N_G * W_G, d))
    return draws, logobj, 3.0 + 0.5 * d * br.LOG_2PI + float(np.log(s).sum()), rng


def _truncated(seed):
    """The standard normal density's kernel in d = 3 on the half space x_0 >= 0.5: log Z = 3/2 log 2 pi + log P(x_0 >= 0.5)."""
    rng = np.random.default_rng(77000 + seed)
    d, a = 3, 0.5
    draws = rng.standard_normal((N_G * W_G, d))
    x0 = rng.standard_normal(8 * N_G * W_G)
    draws[:, 0] = x0[x0 >= a][:N_G * W_G]
    logobj = lambda x: np.where(x[:, 0] >= a, -0.5 * (x * x).sum(axis=1), -np.inf)      # noqa: E731
    return draws, logobj, 1.5 * br.LOG_2PI + math.log(_phi_upper(a)), rng


def _conjugate(seed):
    """y_i ~ N(theta, 1.5^2), i < 12, theta ~ N(1, 2^2): log_obj = log likelihood + log prior, Z the marginal likelihood
    N(y; 1, 1.5^2 I + 2^2 1 1^T), the posterior normal."""
    rng = np.random.default_rng(88000 + seed)
    n, sig, mu0, tau0 = 12, 1.5, 1.0, 2.0
    y = rng.normal(rng.normal(mu0, tau0), sig, n)
    prec = n / sig ** 2 + 1.0 / tau0 ** 2
    pm = (y.sum() / sig ** 2 + mu0 / tau0 ** 2) / prec
    draws = pm + rng.standard_normal((N_G * W_G, 1)) / math.sqrt(prec)

    def logobj(x):
        th = x[:, 0]
        ll = -0.5 * ((y[None, :] - th[:, None]) ** 2).sum(axis=1) / sig ** 2 - n * (math.log(sig) + 0.5 * br.LOG_2PI)
        return ll + (-0.5 * ((th - mu0) / tau0) ** 2 - math.log(tau0) - 0.5 * br.LOG_2PI)

    S = sig ** 2 * np.eye(n) + tau0 ** 2 * np.ones((n, n))
    r = y - mu0
    exact = -0.5 * float(r @ np.linalg.solve(S, r)) - 0.5 * float(np.linalg.slogdet(S)[1]) - 0.5 * n * br.LOG_2PI
    return draws, logobj, exact, rng


def _miss(draws, logobj, exact, rng):
    d = draws.shape[1]
    chain = np.asfortranarray(np.transpose(draws.reshape(N_G, W_G, d), (0, 2, 1)))
    log_obj = logobj(draws).reshape(N_G, W_G)
    r = br.bridge_f64(chain, log_obj, logobj, rng=rng)
    assert r["converged"] and r["iterations"] <= 12 and r["se_logml"] > 0.0
    return abs(r["logml"] - exact) / r["se_logml"], r


@pytest.mark.parametrize("name", ["gaussian_1", "gaussian_2", "gaussian_5", "gaussian_32", "truncated", "conjugate"])
def test_reference_finds_known_marginal_likelihoods(name):
    worst, its = 0.0, set()
    for seed in SEEDS:
        world = _gaussian(int(name.split("_")[1]), seed) if name.startswith("gaussian") else (_truncated if name == "truncated" else _conjugate)(seed)
        z, r = _miss(*world)
        worst = max(worst, z)
        its.add(r["iterations"])
    print(f"[bridge] guard {name}: largest |logml - exact| / se over {len(SEEDS)} seeds = {worst:.2f} (GUARD_Z {br.GUARD_Z}); updates {sorted(its)}")
    assert worst <= br.GUARD_Z


# ---- the sampler's own history ------------------------------------------------------------------------------------------------------
def test_reference_on_the_samplers_history(demc):
    """The target is a normalised density: log Z = 0.  The draws are autocorrelated, so the bound leans on ESS(f2) and on neff."""
    E2E = bc.E2E
    w, prob, chain, log_obj = bc.oracle_history()
    a, b = E2E["window"]
    chain, log_obj = chain[:, :, a - 1:b], log_obj[:, a - 1:b]
    h = (b - a + 1) // 2
    import ess_reference as er
    neff = float(np.median(er.ess(np.asfortranarray(chain[:, :, h:])).ess))
    r = br.bridge_f64(chain, log_obj, lambda x: O.logp(prob, x), seed=demc.bridge_seed(E2E["seed"]), neff=neff, fma=br.fma)
    z = abs(r["logml"]) / r["se_logml"]
    print(f"[bridge] end to end: logml {r['logml']:.4f} (exact 0), se {r['se_logml']:.4f}, miss {z:.2f} se, {r['iterations']} updates, "
          f"neff {neff:.0f} of {r['n_post']}, ESS(f2) {r['ess_f2']:.0f}")
    assert r["converged"] and z <= br.GUARD_Z
