"""demc.jl_amd -- MI355X-native DEMCz chain-update engine behind the call surface of
chrished/DEMC.jl (``demcopt``, ``demcz_sample``, ``demcz_anneal``, ``MC``).

The directory name has a dot, so import it through the repo-root alias module::

    import demc_jl_amd as demc
    mc, Z = demc.demcz_sample(demc.MvNormalTarget(mu, Sigma), Zinit, demc.demcopt(5, N=1024))

All computation below the generation loop runs in ``libdemcz_hip.so`` (HIP, gfx950) through the
C ABI of ``include/demcz.h``; there is no CPU fallback.
"""
from ._lib import DemczError, build, LIB_PATH, SYMBOLS, LAYOUT_SPLIT, LAYOUT_SPLIT_WAVE, LAYOUT_PROGRAM_WAVE          # noqa: F401
from .engine import (HipEngine, CrossoverAdapt, DerivedHistory, selftest_draws, pool_trim, ESS, ess_from_sums, Quantiles, Best, quantile_plan, PPC, ppc_record,
                     select_step, quantile_finish, select_quantiles, RankDiagnostics, rank_to_z,
                     Histogram, Histogram2D, histogram_edges, hdi_steps,
                     LOO, loo_record, loo_compare, psis_tail_length, gpd_fit,
                     Bridge, BridgeIteration, bridge_iterate, bridge_seed, bridge_se, bayes_factor, post_prob,
                     BRIDGE_SEED_XOR)                                                        # noqa: F401
from .targets import MvNormalTarget, IsoQuadTarget, LinRegSSETarget, ProgramTarget, DerivedProgram, PredictiveProgram, PointwiseProgram, is_device_target   # noqa: F401
from .sampler import (MC, DEMCopt, demcopt, demcz_sample, demcz_anneal, tempbaseline,   # noqa: F401
                      make_runner, initial_state,
                      Sharding, DEFAULT_ADAPT)
from .utils import (Rhat_gelman, flatten_chain, accept_ratio, mean_cov_chain, convergence_check,   # noqa: F401
                    save_checkpoint, load_checkpoint, ess_chain, autocov_chain, autocov_sums_chain, posterior_summary,
                    quantile_chain, extract_best, best_logobj, derive_chain, predict_chain, ppc_chain, rank_normalize_chain, rank_diagnostics_chain,
                    pointwise_chain, loo_columns_chain, loo_chain, histogram_chain, histogram2d_chain, hdi_chain,
                    bridge_chain, bridge_posterior_chain, bridge_proposal_program)
from . import workloads                                         # noqa: F401
