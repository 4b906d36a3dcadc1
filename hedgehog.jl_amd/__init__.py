"""MI355X-native Monte Carlo engine behind Hedgehog.jl's `solve(problem, MonteCarlo(...))` API.

Host mirror (Python) of the reference's operator interface for this path; the arithmetic runs in
hand-written HIP kernels behind the C-ABI of include/hedgehog_mc.h (lib/libhedgehog_mc.so).
Import as `hedgehog_jl_amd` (shim at the repository root; the directory name carries a dot).
"""
from . import _ffi, multiasset, routes
from ._ffi import Context, HedgehogMCError, get_context, load_library
from .analytic import (AnalyticSolution, BlackScholesAnalytic, CarrMadan, MertonAnalytic, MultiAssetAnalytic,
                       VarianceGammaAnalytic, merton_series, solve_black_scholes, solve_carr_madan, solve_merton_analytic,
                       solve_multiasset_analytic, solve_vg_analytic, vg_mixing_price)
from .basket import BasketPricingProblem, BasketPricingSolution, solve_basket
from .trees import CoxRossRubinsteinMethod, CRRSolution, solve_crr, solve_crr_basket
from .pde import CrankNicolsonMethod, PDESolution, fd_inputs, solve_pde, solve_pde_basket
from .dates import Date, DateTime, add_years, to_ticks, yearfrac
from .dual import Dual, partials_of, value_of
from .greeks import (AssetSpotLens, AssetVolLens, BatchGreekProblem, CorrelationLens, FDBackward, FDCentral, FDForward,
                     FiniteDifference,
                     ForwardAD, GreekProblem, GreekResult, Pathwise, PropertyLens, SecondOrderGreekProblem, SpotLens,
                     VolLens,
                     ZeroRateSpineLens, optic, set)
from .lsm import (LSM, BoundsSolution, DualBounds, EulerPaths, ExercisePolicy, HestonExactPaths, LSMSolution, SpotPaths,
                  StatePaths, fit_policy, policy_value, simulate_euler_paths, simulate_heston_exact_paths, simulate_spot_paths,
                  simulate_state_paths, solve_dual_bounds, solve_lsm, upper_bound)
from .montecarlo import (AbstractPricingMethod, Antithetic, BatesDynamics, BlackScholesExact, EulerMaruyama,
                         HestonBroadieKaya, HestonDynamics, HestonQE, LognormalDynamics, MertonDynamics, MertonExact, MethodError,
                         MonteCarlo, NoVarianceReduction, NormalLaw, SimulationConfig, VarianceGammaDynamics,
                         VarianceGammaExact, marginal_law,
                         solve_montecarlo, solve_montecarlo_many, solve_path_payoffs)
from .multiasset import (AssetPaths, BestOf, GeometricMean, IndexOption, MultiAssetDynamics, MultiAssetInputs, WeightedSum,
                         WorstOf, simulate_asset_paths, solve_index_lsm, solve_index_options)
from .localvol import (LocalVolDynamics, LocalVolInputs, LocalVolSurface, dupire_from, dupire_local_vol, get_local_vol,
                       refuse_other_methods, solve_localvol_payoffs)
from .qmc import (BrownianBridge, Incremental, QuasiMonteCarlo, QuasiMonteCarloSolution, SobolConfig, solve_qmc)
from .mlmc import MLMCConfig, MultilevelLevel, MultilevelMonteCarlo, MultilevelSolution, solve_mlmc
from .distributed import rank_device, shard_range, solve_lsm_sharded, solve_sharded
from .domain import (American, ArithmeticAverage, AsianOption, AssetOrNothing, BarrierOption, BatesInputs, BlackScholesInputs,
                    Call, CashOrNothing, ContinuousMonitoring, DigitalOption, DownAndIn, DownAndOut, European,
                    FlatRateCurve, FlatVolSurface, Forward, GeometricAverage, HestonInputs, LookbackOption, MertonInputs,
                    Monitoring,
                    MonteCarloSolution,
                    PricingProblem, Put, RateCurve, Spot, UpAndIn, UpAndOut, VanillaOption, VarianceGammaInputs, df, df_yf,
                    get_vol,
                    spine_zeros, zero_rate, zero_rate_yf)


def solve(*args, **kw):
    """The reference's single verb (src/Hedgehog.jl:59-98), for the methods on the hot path:

        solve(prob::PricingProblem, method::MonteCarlo)                      montecarlo.jl:478
        solve(prob::PricingProblem{AsianOption | BarrierOption | DigitalOption | LookbackOption}, method::MonteCarlo)
                                                  (Euler paths; barriers and lookbacks also ContinuousMonitoring())
        solve(gprob::GreekProblem, ::ForwardAD, method)                      greeks_problem.jl:249
        solve(gprob::GreekProblem, ::FiniteDifference, method)               greeks_problem.jl:318
        solve(gprob::GreekProblem | ::BatchGreekProblem, ::Pathwise, ::MonteCarlo(…, EulerMaruyama(), …))
                                  pathwise Greeks of Asian / lookback / vanilla payoffs, one pass (no reference method)
        solve(gprob::SecondOrderGreekProblem, ::FiniteDifference, method)    greeks_problem.jl:396
        solve(gprob::BatchGreekProblem, ::GreekMethod, method)               greeks_problem.jl:559
        solve(prob::BasketPricingProblem, method::MonteCarlo | ::CarrMadan)  basket.jl:35
        solve(prob, ::CarrMadan) / solve(prob, ::BlackScholesAnalytic)       carr_madan.jl:47, black_scholes.jl:38
        solve(prob::PricingProblem{…, MertonInputs}, ::MonteCarlo(MertonDynamics(), MertonExact() | EulerMaruyama(), …)
              | ::CarrMadan(α, bound, MertonDynamics()) | ::MertonAnalytic)   Merton jump diffusion (no reference method)
        solve(prob::PricingProblem{…, HestonInputs}, ::MonteCarlo(HestonDynamics(), HestonQE(psi_c, martingale), …))
                                                                              Andersen's QE scheme (no reference method)
        solve(prob::PricingProblem{…, BatesInputs}, ::MonteCarlo(BatesDynamics(), HestonQE(psi_c, martingale), …)
              | ::CarrMadan(α, bound, BatesDynamics()))   Bates: Heston QE paths with Merton jumps (no reference method)
        solve(prob::PricingProblem{…, VarianceGammaInputs} | ::BasketPricingProblem,
              ::MonteCarlo(VarianceGammaDynamics(), VarianceGammaExact(), …) | ::CarrMadan(α, bound, VarianceGammaDynamics())
              | ::VarianceGammaAnalytic)   Variance Gamma: gamma time-changed paths, exact on any dates (no reference method)
        solve(prob::PricingProblem{IndexOption, MultiAssetInputs} | ::BasketPricingProblem of IndexOptions,
              ::MonteCarlo(MultiAssetDynamics(), EulerMaruyama(), …) | ::MultiAssetAnalytic)
                                  several correlated assets: baskets, spreads, best-of / worst-of (no reference method)
        solve(prob::PricingProblem{…, LocalVolInputs} | ::BasketPricingProblem,
              ::MonteCarlo(LocalVolDynamics(), EulerMaruyama(), …))
                                  local volatility on a tabulated surface, Dupire's formula beside it (no reference method)
        solve(prob::PricingProblem{<:VanillaOption{…,European,…,Spot}}, ::QuasiMonteCarlo(dynamics, strategy, SobolConfig(…)))
                                  randomised Sobol' points through the REPLAY solve: LognormalDynamics with BlackScholesExact
                                  or EulerMaruyama, HestonDynamics with EulerMaruyama (no reference method)
        solve(prob::PricingProblem, ::MultilevelMonteCarlo(dynamics, EulerMaruyama(), MLMCConfig(steps, …)))
                                  multilevel Monte Carlo on coupled Euler levels of steps·2^l steps: European vanillas and the
                                  path-dependent payoffs under a Monitoring, lognormal or Heston (no reference method)
        solve(prob::PricingProblem{<:VanillaOption{…,American,…}}, ::LSM)     least_squares_montecarlo.jl:99
        solve(prob::PricingProblem{IndexOption{…, VanillaOption{…,American,…}}, MultiAssetInputs},
              ::LSM(MultiAssetDynamics(), EulerMaruyama(), config, degree); exercise_every=m)
                                  American / Bermudan baskets and rainbows: a regression basis in several variables
        solve(prob::PricingProblem{<:VanillaOption{…,American,…}}, ::LSM; exercise_every=m, regressors="spot_variance")
                                  Heston Euler (path_state="spot"), HestonQE, Bates: the regression on spot AND variance
        solve(prob::PricingProblem{<:VanillaOption{…,American,…}, HestonInputs},
              ::DualBounds(LSM(HestonDynamics(), EulerMaruyama(), config, degree), outer=, inner=, fresh=, inner_seed=); exercise_every=m)
                                  the bracket: the fitted policy on fresh paths (lower), the Andersen–Broadie dual (upper)
        solve(prob::PricingProblem{<:VanillaOption}, ::CoxRossRubinsteinMethod) cox_ross_rubinstein.jl:99
        solve(prob::BasketPricingProblem, ::CoxRossRubinsteinMethod)         basket.jl:35
        solve(prob::PricingProblem{<:VanillaOption} | ::BasketPricingProblem, ::CrankNicolsonMethod)
                                                  (a Crank–Nicolson grid per option; no reference method)
    """
    from . import greeks as _g
    if len(args) == 2 and isinstance(args[0], (PricingProblem, BasketPricingProblem)) and isinstance(args[1], QuasiMonteCarlo):
        from .qmc import SUPPORTED  # every refusal of this method names what it does price
        if not isinstance(args[0], PricingProblem):
            raise MethodError(f"a basket has no many-strike quasi-Monte Carlo form: {SUPPORTED}")
        if kw:
            raise MethodError(f"QuasiMonteCarlo fills its own REPLAY buffer and takes no {sorted(kw)}: {SUPPORTED}")
        return solve_qmc(args[0], args[1])
    if len(args) == 2 and isinstance(args[0], (PricingProblem, BasketPricingProblem)) and isinstance(args[1], MultilevelMonteCarlo):
        from .mlmc import check_supported  # every refusal of this method names what it does price
        check_supported(args[0], args[1], kw)
        return solve_mlmc(args[0], args[1])
    if len(args) == 2 and isinstance(args[0], (PricingProblem, BasketPricingProblem)):
        payoffs = multiasset.payoffs_of(args[0])
        if isinstance(args[0], PricingProblem) and isinstance(args[1], MultiAssetAnalytic) and \
                multiasset.is_multiasset(payoffs, args[0].market_inputs, args[1]):
            return solve_multiasset_analytic(args[0], args[1])
        routes.refuse_other_methods(payoffs, args[0].market_inputs, args[1])  # a model with routes of its own: them, or a MethodError naming them
    if len(args) == 2 and isinstance(args[0], PricingProblem) and isinstance(args[1], MonteCarlo):
        return solve_montecarlo(args[0], args[1], **kw)
    if len(args) == 2 and isinstance(args[0], PricingProblem) and isinstance(args[1], CarrMadan):
        return solve_carr_madan(args[0], args[1])
    if len(args) == 2 and isinstance(args[0], PricingProblem) and \
            isinstance(args[1], BlackScholesAnalytic):
        return solve_black_scholes(args[0], args[1])
    if len(args) == 2 and isinstance(args[0], PricingProblem) and isinstance(args[1], VarianceGammaAnalytic):
        return solve_vg_analytic(args[0], args[1])
    if len(args) == 2 and isinstance(args[0], PricingProblem) and isinstance(args[1], MertonAnalytic):
        return solve_merton_analytic(args[0], args[1])
    if len(args) == 2 and isinstance(args[0], PricingProblem) and isinstance(args[1], LSM):
        return solve_lsm(args[0], args[1], **kw)
    if len(args) == 2 and isinstance(args[0], PricingProblem) and isinstance(args[1], DualBounds):
        return solve_dual_bounds(args[0], args[1], **kw)
    if len(args) == 2 and isinstance(args[0], PricingProblem) and isinstance(args[1], CoxRossRubinsteinMethod):
        return solve_crr(args[0], args[1])
    if len(args) == 2 and isinstance(args[0], PricingProblem) and isinstance(args[1], CrankNicolsonMethod):
        return solve_pde(args[0], args[1])
    if len(args) == 2 and isinstance(args[0], BasketPricingProblem) and \
            isinstance(args[1], (MonteCarlo, CarrMadan, CoxRossRubinsteinMethod, CrankNicolsonMethod)):
        return solve_basket(args[0], args[1], **kw)
    if len(args) == 3 and isinstance(args[0], GreekProblem):
        if isinstance(args[1], ForwardAD):
            return _g.solve_greek_ad(args[0], args[2], solve)
        if isinstance(args[1], FiniteDifference):
            return _g.solve_greek_fd(args[0], args[1], args[2], solve)
        if isinstance(args[1], Pathwise):
            lens = args[0].wrt
            return GreekResult(_g.solve_pathwise(args[0].pricing_problem, (lens,), args[2], solve, kw)[lens])
    if len(args) == 3 and isinstance(args[0], SecondOrderGreekProblem) and \
            isinstance(args[1], FiniteDifference):
        return _g.solve_second_order_fd(args[0], args[1], args[2], solve)
    if len(args) == 3 and isinstance(args[0], BatchGreekProblem):
        return _g.solve_batch(args[0], args[1], args[2], solve, **(kw if isinstance(args[1], Pathwise) else {}))
    raise MethodError("no method matching solve(" + ", ".join(type(a).__name__ for a in args) + ")")
