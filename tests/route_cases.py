"""What the Python host sends to the C-ABI, route by route, without a GPU: a recording context in place of
_ffi.get_context, and the table of cases whose records tests/golden/route_pins.json holds.

The file holds a SHA-256 per record and every refusal text in full (`pins`); `make_route_pins.py --full PATH` writes the
records themselves, to compare two commits field by field.

A record is what one call of the public API did: the entry points it reached, in order, with every argument — structs as
their non-zero fields and a SHA-256 of their bytes (addresses zeroed; what a pointer points to is listed in its place: the
partials of an hh_model, the times and vols of an hh_localvol), arrays of hh_path_payoff element by element, host
addresses as "given" or "NULL", scalars as they are — and either what came back (the prices the recorder wrote, 100 · call
+ k, so the order of the solutions shows; the ensemble's shape and whether it is the array the call was given) or the
exception's type and text.

Every route is recorded with ensemble true and false: the plain terminal route keeps its samples in a DeviceBuffer, which
the context fakes with one address from its pool (`pool_take`); its ensemble is recorded as "device", unread.
The multi-GPU successes (`devices=` on the plain route and its basket) are not recorded: MultiGpu's solve, solve_multi and
check would each need a fake of their own; tests/test_gpu_mgpu.py holds them.

This module and tests/golden/make_route_pins.py use the package's public names only, so that the pins can be rewritten
from any earlier commit and compared byte for byte."""
import contextlib
import ctypes as C
import hashlib
import json
import os

import numpy as np

import hedgehog_jl_amd as hh
from hedgehog_jl_amd import _ffi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_pins.json")
REF, EXP, LATER = hh.Date(2021, 1, 1), hh.Date(2022, 1, 1), hh.Date(2023, 1, 1)
ADDRESS = 1 << 20  # integers from here on are addresses; the fake seed and pool addresses lie below


# ---- the recorder ------------------------------------------------------------------------------------------------------------

def _pointed(x, name, P):
    if isinstance(x, _ffi.hh_localvol):
        return x.n_times if name == "times" else x.n_times * x.n_x
    return P  # hh_model: the partials


def dump_struct(x, P=0):
    out, clean = {}, type(x).from_buffer_copy(bytes(x))
    for name, ftype in x._fields_:
        v = getattr(x, name)
        if ftype is _ffi._dp:
            if v:
                out[name] = [v[i] for i in range(_pointed(x, name, P))]
                setattr(clean, name, None)
        elif ftype is C.c_void_p:
            if v is not None:
                out[name] = v if v < ADDRESS else "given"
                if v >= ADDRESS:
                    setattr(clean, name, None)
        elif isinstance(v, C.Array):
            if any(v):
                out[name] = list(v)
        elif v != 0:
            out[name] = v
    out["sha"] = hashlib.sha256(bytes(clean)).hexdigest()[:16]
    return out


class RecordingLib:
    def __init__(self, log=True):
        self.calls, self.addresses, self.log = [], set(), log

    def hh_seeds_fingerprint(self, ptr, n):
        return 1

    def __getattr__(self, entry):
        def call(*args):
            if not self.log:  # a timing run: the host's own work alone
                return 0
            objs = [getattr(a, "_obj", a) for a in args]
            P = next((o.n_partials for o in objs if isinstance(o, _ffi.hh_config)), 0)
            no = len(self.calls) + 1
            self.calls.append({"entry": entry, "args": [self._dump(o, P, no) for o in objs]})
            return 0
        return call

    def _dump(self, a, P, no):
        if a is None:
            return "NULL"
        if isinstance(a, _ffi.hh_result):
            a.price, a.std_error = 100.0 * no, 0.5
            return "result"
        if isinstance(a, C.Structure):
            return dump_struct(a, P)
        if isinstance(a, C.Array):
            if a._type_ is _ffi.hh_result:
                for k in range(len(a)):
                    a[k].price, a[k].std_error = 100.0 * no + k, 0.5
                return f"results[{len(a)}]"
            return [dump_struct(e, P) for e in a] if issubclass(a._type_, C.Structure) else list(a)
        if isinstance(a, int) and not isinstance(a, bool) and a >= 4096:
            self.addresses.add(a)
            return "given"
        return a if isinstance(a, (int, float)) else type(a).__name__


class RecordingCtx:
    handle = None

    def __init__(self, log=True):
        self.lib = RecordingLib(log)

    def check(self, rc):
        assert rc == 0

    def seeds_on_device(self, seeds, fingerprint=0):
        return 4096

    def pool_take(self, nbytes):
        return 8192


def _no_multi_gpu(*a, **k):
    raise RuntimeError("the multi-GPU routes are not recorded")


@contextlib.contextmanager
def recording(log=True):
    ctx, saved = RecordingCtx(log), (_ffi.get_context, _ffi.get_multi_gpu)
    _ffi.get_context, _ffi.get_multi_gpu = (lambda device=0: ctx), _no_multi_gpu
    try:
        yield ctx.lib
    finally:
        _ffi.get_context, _ffi.get_multi_gpu = saved


def _ensemble(sol, lib):
    ens = object.__getattribute__(sol, "ensemble")
    if ens is None:
        return None
    if isinstance(ens, tuple):
        return {"shapes": [list(e.shape) for e in ens], "given": ens[0].ctypes.data in lib.addresses}
    if isinstance(ens, np.ndarray):
        return {"shape": list(ens.shape), "given": ens.ctypes.data in lib.addresses}
    return "device"


def describe(out, lib):
    if isinstance(out, hh.BasketPricingSolution):
        out = list(out.solutions)
    if isinstance(out, list):
        return [describe(s, lib) for s in out]
    if isinstance(out, hh.MonteCarloSolution):
        price = out.price
        if isinstance(price, hh.Dual):
            price = {"value": hh.value_of(price), "partials": list(hh.partials_of(price, len(price.partials)))}
        return {"price": price, "std_error": out.std_error, "ensemble": _ensemble(out, lib)}
    return out if out is None else type(out).__name__


def run(fn):
    with recording() as lib:
        try:
            out = describe(fn(), lib)
        except Exception as e:  # noqa: BLE001 — the record is the exception
            return {"raises": [type(e).__name__, str(e)], "calls": lib.calls}
    return {"out": out, "calls": lib.calls}


# ---- payoffs, markets, methods ----------------------------------------------------------------------------------------------------

M3 = hh.Monitoring(3, True)
DUAL = lambda v: hh.Dual(v, (1.0,))  # noqa: E731


def vanilla(K=100.0, expiry=EXP, style=None, cp=None):
    return hh.VanillaOption(K, expiry, style or hh.European(), cp or hh.Call(), hh.Spot())


def asian(K=100.0, expiry=EXP, mon=M3):
    return hh.AsianOption(K, expiry, hh.Call(), hh.ArithmeticAverage(), mon)


def barrier(mon=M3, barrier=115.0, rebate=1.0, expiry=EXP):
    return hh.BarrierOption(100.0, barrier, expiry, hh.Call(), hh.UpAndOut(), rebate=rebate, monitoring=mon)


def eight_payoffs():
    """the payoffs of tests/test_gpu_path_payoff.python_payoffs()"""
    return [hh.AsianOption(100.0, EXP, hh.Call(), hh.ArithmeticAverage(), M3),
            hh.AsianOption(100.0, EXP, hh.Put(), hh.GeometricAverage(), M3),
            hh.BarrierOption(100.0, 115.0, EXP, hh.Call(), hh.UpAndOut(), rebate=1.0, monitoring=M3),
            hh.BarrierOption(100.0, 115.0, EXP, hh.Call(), hh.UpAndIn(), rebate=1.0, monitoring=M3),
            hh.BarrierOption(100.0, 90.0, EXP, hh.Put(), hh.DownAndOut(), monitoring=M3),
            hh.BarrierOption(100.0, 90.0, EXP, hh.Put(), hh.DownAndIn(), monitoring=M3),
            hh.DigitalOption(100.0, EXP, hh.Call(), hh.CashOrNothing(5.0)),
            hh.DigitalOption(100.0, EXP, hh.Put(), hh.AssetOrNothing())]


def bs(r=0.03, S=100.0, sigma=0.2):
    return hh.BlackScholesInputs(REF, r, S, sigma)


def heston(r=0.03, S=100.0, V0=0.04, k=2.0, th=0.05, s=0.3, rho=-0.7):
    return hh.HestonInputs(REF, r, S, V0, k, th, s, rho)


def merton(r=0.03, S=100.0, sigma=0.2, lam=0.8, mu=-0.1, std=0.15):
    return hh.MertonInputs(REF, r, S, sigma, lam, mu, std)


def bates(r=0.03, S=100.0, V0=0.04, k=0.3, th=0.05, s=0.9, rho=-0.5, lam=0.8, mu=-0.1, std=0.15):
    return hh.BatesInputs(REF, r, S, V0, k, th, s, rho, lam, mu, std)


SURFACE = hh.LocalVolSurface([0.25, 1.0], [4.0, 4.5, 5.0], [[0.3, 0.2, 0.25], [0.28, 0.22, 0.24]])


def localvol(r=0.03, S=100.0):
    return hh.LocalVolInputs(REF, r, S, SURFACE)


CORR = [[1.0, 0.5, -0.2], [0.5, 1.0, 0.1], [-0.2, 0.1, 1.0]]
WEIGHTS = (0.5, 0.3, 0.2)
INDEX = hh.WeightedSum(WEIGHTS)


def assets(r=0.03, spots=(100.0, 90.0, 110.0), sigmas=(0.2, 0.35, 0.25), corr=CORR):
    return hh.MultiAssetInputs(REF, r, spots, sigmas, corr)


def on_index(p):
    return hh.IndexOption(INDEX, p)


def mc(dyn, strat, steps=4, n=8, anti=False, **kw):
    cfg = hh.SimulationConfig(n, steps=steps, seeds=np.arange(1, n + 1, dtype=np.uint64),
                              variance_reduction=hh.Antithetic() if anti else hh.NoVarianceReduction())
    return hh.MonteCarlo(dyn, strat, cfg, **kw)


def execute(s):
    """one call of the public API on a spec: a dict of how, payoffs, market, dyn, strat, steps, anti, mkw, skw, method"""
    method = s.get("method") or mc(s["dyn"], s["strat"], s["steps"], anti=s.get("anti", False), **s.get("mkw", {}))
    wrap = s.get("wrap") or (lambda p: p)
    payoffs, mkt, skw = [wrap(p) for p in s["payoffs"]], s["market"], s.get("skw", {})
    how = s.get("how", "single")
    if how == "single":
        return hh.solve(hh.PricingProblem(payoffs[0], mkt), method, **skw)
    if how == "basket":
        return hh.solve(hh.BasketPricingProblem(payoffs, mkt), method, **skw)
    if how == "group":  # the route's public function for payoffs on ONE simulation
        return s["group"](payoffs, mkt, method, **skw)
    assert how == "many"
    return hh.solve_montecarlo_many([hh.PricingProblem(p, mkt) for p in payoffs], method, **skw)


def route(payoff, market, dyn, strat, steps, wrong, duals, group=hh.solve_path_payoffs, wrap=None, other=False, path=True):
    return dict(spec=dict(payoffs=[payoff], market=market(), dyn=dyn, strat=strat, steps=steps, group=group, wrap=wrap),
                make_market=market, wrong=wrong, duals=duals, other=other, path=path)


ALL_BS, ALL_HESTON = ("r", "S", "sigma"), ("r", "S", "V0", "k", "th", "s", "rho")
ROUTES = {
    "plain": route(vanilla(), bs, hh.LognormalDynamics(), hh.BlackScholesExact(), 1,
                   dict(dyn=hh.HestonDynamics(), strat=hh.HestonBroadieKaya(), market=heston()), ALL_BS, path=False),
    "plain_euler": route(vanilla(), heston, hh.HestonDynamics(), hh.EulerMaruyama(), 4,
                         dict(dyn=hh.LognormalDynamics(), strat=hh.BlackScholesExact(), market=bs()), ALL_HESTON, path=False),
    "euler": route(asian(), heston, hh.HestonDynamics(), hh.EulerMaruyama(), 12,
                   dict(dyn=hh.LognormalDynamics(), strat=hh.HestonBroadieKaya(), market=bs()), ALL_HESTON),
    "merton": route(asian(), merton, hh.MertonDynamics(), hh.EulerMaruyama(), 12,
                    dict(dyn=hh.LognormalDynamics(), strat=hh.BlackScholesExact(), market=bs()), ALL_BS + ("lam", "mu", "std")),
    "merton_exact": route(vanilla(), merton, hh.MertonDynamics(), hh.MertonExact(), 1,
                          dict(dyn=hh.LognormalDynamics(), strat=hh.BlackScholesExact(), market=bs()), ALL_BS + ("lam", "mu", "std"),
                          path=False),
    "qe": route(asian(), heston, hh.HestonDynamics(), hh.HestonQE(1.25, True), 12,
                dict(dyn=hh.LognormalDynamics(), strat=None, market=bs()), ALL_HESTON),
    "bates": route(asian(), bates, hh.BatesDynamics(), hh.HestonQE(), 12,
                   dict(dyn=hh.HestonDynamics(), strat=hh.EulerMaruyama(), market=heston()), ALL_HESTON + ("lam", "mu", "std"),
                   other=True),
    "localvol": route(barrier(), localvol, hh.LocalVolDynamics(), hh.EulerMaruyama(), 12,
                      dict(dyn=hh.LognormalDynamics(), strat=hh.BlackScholesExact(), market=bs()), ("r", "S"),
                      group=hh.solve_localvol_payoffs, other=True),
    "multiasset": route(asian(), assets, hh.MultiAssetDynamics(), hh.EulerMaruyama(), 12,
                        dict(dyn=hh.LognormalDynamics(), strat=hh.BlackScholesExact(), market=bs()), ("r",),
                        group=hh.solve_index_options, wrap=on_index, other=True),
}


def faults(name):
    """{fault: change of the route's spec}, one fault each; None where the route has no such fault"""
    r = ROUTES[name]
    steps = r["spec"]["steps"]
    f = {"wrong_dynamics": dict(dyn=r["wrong"]["dyn"]), "wrong_inputs": dict(market=r["wrong"]["market"])}
    if r["wrong"]["strat"] is not None:
        f["wrong_strategy"] = dict(strat=r["wrong"]["strat"])
    f["replay"] = dict(skw=dict(replay=np.zeros((8, steps, 2))))
    if name not in ("plain", "plain_euler"):  # there `devices=` is the multi-GPU solve (not recorded)
        f["devices"] = dict(mkw=dict(devices=(0,)))
    for field in r["duals"]:
        default = r["make_market"].__defaults__[r["make_market"].__code__.co_varnames.index(field)]
        f["dual_" + field] = dict(market=r["make_market"](**{field: DUAL(default)}))
    if name == "multiasset":
        f["dual_spot"] = dict(market=assets(spots=(DUAL(100.0), 90.0, 110.0)))
        f["dual_sigma"] = dict(market=assets(sigmas=(0.2, DUAL(0.35), 0.25)))
        f["dual_corr"] = dict(market=assets(corr=[[1.0, DUAL(0.5), -0.2], [DUAL(0.5), 1.0, 0.1], [-0.2, 0.1, 1.0]]))
        f["dual_weight"] = dict(wrap=lambda p: hh.IndexOption(hh.WeightedSum((DUAL(0.5), 0.3, 0.2)), p))
    f["dual_strike"] = dict(payoffs=[vanilla(DUAL(100.0))])
    f["dual_asian_strike"] = dict(payoffs=[asian(DUAL(100.0))])
    f["dual_barrier"] = dict(payoffs=[barrier(barrier=DUAL(115.0))])
    f["dual_rebate"] = dict(payoffs=[barrier(rebate=DUAL(1.0))])
    f["dual_cash"] = dict(payoffs=[hh.DigitalOption(100.0, EXP, hh.Call(), hh.CashOrNothing(DUAL(5.0)))])
    f["american"] = dict(payoffs=[vanilla(style=hh.American())])
    f["continuous_barrier"] = dict(payoffs=[barrier(mon=hh.ContinuousMonitoring())])
    f["continuous_lookback"] = dict(payoffs=[hh.LookbackOption(EXP, hh.Call(), monitoring=hh.ContinuousMonitoring())])
    f["two_expiries"] = dict(how="group", payoffs=[asian(), asian(expiry=LATER)])
    f["two_monitorings"] = dict(how="group", payoffs=[asian(), asian(mon=hh.Monitoring(1))])
    f["two_extremes"] = dict(how="group", payoffs=[barrier(), barrier(mon=hh.ContinuousMonitoring())])
    f["every_not_dividing"] = dict(payoffs=[asian(mon=hh.Monitoring(5))])
    f["path_payoff"] = dict(payoffs=[asian()])  # a fault on the terminal routes only
    return f


def other_methods():
    cfg = hh.SimulationConfig(8, steps=4, seeds=np.arange(1, 9, dtype=np.uint64))
    return {"BlackScholesAnalytic": hh.BlackScholesAnalytic(), "MertonAnalytic": hh.MertonAnalytic(),
            "MultiAssetAnalytic": hh.MultiAssetAnalytic(), "CarrMadan_lognormal": hh.CarrMadan(1.0, 32.0, hh.LognormalDynamics()),
            "CarrMadan_heston": hh.CarrMadan(1.0, 32.0, hh.HestonDynamics()), "CarrMadan_merton": hh.CarrMadan(1.0, 32.0, hh.MertonDynamics()),
            "LSM": hh.LSM(hh.HestonDynamics(), hh.EulerMaruyama(), cfg, 2), "CRR": hh.CoxRossRubinsteinMethod(10),
            "CrankNicolson": hh.CrankNicolsonMethod(20, 20)}


def baskets():
    """{name: spec} of the basket cases"""
    daily = hh.BarrierOption(100.0, 115.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=hh.Monitoring(1))
    host = [hh.AsianOption(100.0, EXP, hh.Call(), monitoring=hh.Monitoring(2)), vanilla(95.0), hh.DigitalOption(101.0, EXP, hh.Put()),
            vanilla(110.0, LATER, cp=hh.Put()), hh.BarrierOption(100.0, 80.0, EXP, hh.Call(), hh.DownAndOut(), monitoring=hh.Monitoring(2))]
    pair = [vanilla(96.0), vanilla(106.0)]
    mon = hh.Monitoring(1, False)
    index_opts = [hh.IndexOption(INDEX, vanilla(100.0)), hh.IndexOption(hh.WorstOf(), vanilla(95.0, cp=hh.Put())),
                  hh.IndexOption(hh.WeightedSum(tuple(WEIGHTS)), hh.AsianOption(100.0, EXP, hh.Call(), monitoring=mon)),
                  hh.IndexOption(INDEX, hh.BarrierOption(100.0, 130.0, EXP, hh.Call(), hh.UpAndOut(), monitoring=mon)),
                  hh.IndexOption(hh.WeightedSum((1.0, -1.0, 0.0)), vanilla(5.0))]
    out = {}
    for name, payoffs, r, kw in (
            ("euler_mixed", eight_payoffs() + [vanilla(), daily], "euler", dict(anti=True)),
            ("euler_bridge", [barrier(), barrier(mon=hh.ContinuousMonitoring()), asian(), hh.LookbackOption(EXP, hh.Call()), vanilla(),
                              vanilla(90.0, LATER)], "euler", {}),
            ("plain_two_expiries", [vanilla(95.0), vanilla(105.0, cp=hh.Put()), vanilla(100.0, LATER), vanilla(DUAL(100.0))], "plain", {}),
            ("plain_dual_spot", pair, "plain", dict(market=bs(S=DUAL(100.0)))),
            ("plain_euler_pair", pair, "plain_euler", dict(anti=True)),
            ("bates_host", host, "bates", {}), ("bates_pair", pair, "bates", {}),
            ("bates_wrong_strategy", pair, "bates", dict(strat=hh.EulerMaruyama())),
            ("qe_host", host, "qe", {}), ("qe_pair", pair, "qe", {}),
            ("merton_host", host, "merton", {}), ("merton_pair", pair, "merton", {}),
            ("merton_exact_pair", [vanilla(95.0), vanilla(105.0, cp=hh.Put())], "merton_exact", {}),
            ("localvol_groups", [barrier(), vanilla(95.0), vanilla(110.0, LATER, cp=hh.Put()), barrier(mon=hh.ContinuousMonitoring()),
                                 vanilla(90.0, LATER), asian(mon=hh.Monitoring(2))], "localvol", {}),
            ("localvol_american", [vanilla(style=hh.American()), barrier()], "localvol", {}),
            ("localvol_wrong_dynamics", [barrier(), vanilla()], "localvol", dict(dyn=hh.LognormalDynamics())),
            ("multiasset_indices", index_opts, "multiasset", dict(steps=6, wrap=None)),
            ("multiasset_bare_payoff", [index_opts[0], vanilla()], "multiasset", dict(wrap=None))):
        for ens in (False, True):
            out[f"{name}/ensemble={ens}"] = dict(ROUTES[r]["spec"], how="basket", payoffs=payoffs, skw=dict(ensemble=ens), **kw)
    return out


def cases():
    """{id: spec} — every record of the pin file"""
    out = {}
    for name, r in ROUTES.items():
        good = r["spec"]
        singles = {"good": good["payoffs"][0]}
        if r["path"]:
            singles["vanilla"] = vanilla()
        if name == "euler":
            singles.update({f"kind{k}": p for k, p in enumerate(eight_payoffs())})
        if name in ("euler", "localvol"):
            singles.update(lookback=hh.LookbackOption(EXP, hh.Call(), monitoring=M3), lookback_fixed=hh.LookbackOption(EXP, hh.Put(), 100.0, M3),
                           continuous_barrier=barrier(mon=hh.ContinuousMonitoring()),
                           continuous_lookback=hh.LookbackOption(EXP, hh.Call(), monitoring=hh.ContinuousMonitoring()))
        for tag, p in singles.items():
            for ens in (False, True):
                for anti in (False, True):
                    out[f"{name}/single/{tag}/ensemble={ens}/antithetic={anti}"] = dict(good, payoffs=[p], anti=anti, skw=dict(ensemble=ens))
        f = faults(name)
        for tag, change in f.items():
            out[f"{name}/fault/{tag}"] = dict(good, **change)
        for wrong in ("wrong_dynamics", "wrong_strategy", "wrong_inputs"):
            for tag, change in f.items():
                if wrong in f and not tag.startswith("wrong_") and not (tag.startswith("dual_") and "market" in change and wrong == "wrong_inputs"):
                    out[f"{name}/fault/{wrong}+{tag}"] = dict(good, **dict(f[wrong], **change))
        out[f"{name}/many/vanillas"] = dict(good, how="many", payoffs=[vanilla(95.0), vanilla(105.0)])
        out[f"{name}/many/good"] = dict(good, how="many", payoffs=[good["payoffs"][0]] * 2)
        if r["other"]:
            for tag, method in other_methods().items():
                out[f"{name}/other/{tag}"] = dict(good, method=method)
                out[f"{name}/other/{tag}/basket"] = dict(good, method=method, how="basket")
    plain = ROUTES["plain"]["spec"]
    for tag, kw in (("lognormal_euler", dict(strat=hh.EulerMaruyama(), steps=4)), ("heston_bk", dict(ROUTES["plain_euler"]["spec"], strat=hh.HestonBroadieKaya(), steps=1)),
                    ("compat_sqrt_alpha", dict(mkw=dict(compat_sqrt_alpha=True, em_split=False))), ("put", dict(payoffs=[vanilla(cp=hh.Put())]))):
        out[f"plain/single/{tag}"] = dict(plain, **kw)
    out["plain/many/replay"] = dict(plain, how="many", payoffs=[vanilla(95.0), vanilla(105.0)], skw=dict(replay=np.zeros((8, 1, 1))))
    out["plain/many/dual"] = dict(plain, how="many", payoffs=[vanilla(95.0), vanilla(DUAL(105.0))])
    out["plain/many/one"] = dict(plain, how="many", payoffs=[vanilla(95.0)])
    out["plain/many/devices_replay"] = dict(plain, how="many", payoffs=[vanilla(95.0), vanilla(105.0)], mkw=dict(devices=(0, 1)),
                                            skw=dict(replay=np.zeros((8, 1, 1))))
    out.update({"basket/" + k: v for k, v in baskets().items()})
    return out


def compute():
    """{id: record}, through JSON so that floats and tuples read as they would from a file"""
    return json.loads(json.dumps({cid: run(lambda s=s: execute(s)) for cid, s in cases().items()}))


def pins(records):
    """What the file holds of the records: every distinct refusal text, readable, and per record the first 12 hex digits of
    the SHA-256 of its canonical JSON, grouped by the first two parts of the id (a route and a kind of case)."""
    doc = {"messages": sorted({r["raises"][1] for r in records.values() if "raises" in r}), "pins": {}}
    for cid in sorted(records):
        route, kind, tag = cid.split("/", 2)
        group = route + "/" + kind
        digest = hashlib.sha256(json.dumps(records[cid], sort_keys=True).encode()).hexdigest()[:12]
        doc["pins"].setdefault(group, {})[tag] = digest
    return doc


def dump(doc):
    """the file's text: one message per line, one group of pins per line"""
    groups = [f"{json.dumps(g)}: {json.dumps(d, sort_keys=True)}" for g, d in sorted(doc["pins"].items())]
    return ('{"messages": [\n' + ",\n".join(json.dumps(m, ensure_ascii=False) for m in doc["messages"]) + '\n],\n"pins": {\n' +
            ",\n".join(groups) + "\n}}\n")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
