"""The Julia layer has never run (no toolchain here), so its dispatch is checked by reading it: two methods of one
function that overlap in their arguments, each more specific in a different one, make every call in the overlap an
ambiguity error, and Julia does not dispatch on keywords.  The methods of `solve_lsm_hip` are kept apart by the
simulation strategy their `method` argument names."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIA = os.path.join(ROOT, "julia", "HedgehogMC.jl")
STRATEGIES = {"BlackScholesExact", "EulerMaruyama", "HestonBroadieKaya"}


def _signatures(name):
    src = open(JULIA).read()
    return re.findall(r"^function " + name + r"\((.*?)\)\s*where", src, re.S | re.M)


def test_every_lsm_method_names_its_own_strategy():
    sigs = _signatures("solve_lsm_hip")
    assert len(sigs) >= 2
    named = []
    for sig in sigs:
        m = re.search(r"method::Hedgehog\.LSM\{(.*?)\}\s*[;,)]", sig + ")", re.S)
        assert m, f"a solve_lsm_hip method whose `method` argument names no MonteCarlo type:\n{sig}"
        # MonteCarlo{dynamics, strategy, config}: the strategy is the second parameter
        mc = re.search(r"MonteCarlo\{([^,{}]+),\s*([^,{}]+)", m.group(1))
        assert mc, sig
        strategy = mc.group(2).strip()
        assert strategy in STRATEGIES, (strategy, sig)
        named.append(strategy)
    assert len(named) == len(set(named)), f"two solve_lsm_hip methods for one strategy: {named}"
