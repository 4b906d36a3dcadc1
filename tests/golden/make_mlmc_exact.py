"""Writes tests/golden/mlmc_exact.json: what the numpy restatement of tests/mlmc_cases.py — the split-step Euler scheme on
numpy's normals, a fine and a coarse trajectory on the same increments — gives for the mild Heston case on steps 4, 8, 16,
32 with the device tests' trajectories per level (2^18, 2^16, 2^15, 2^14), on two seeds: the mean and the variance of P_0 and of every correction P_l − P_{l−1}
(undiscounted), for the call and the arithmetic Asian call on 4 dates.  The conditions of tests/test_gpu_mlmc.py's coupling
test — V_1 <= Var(P_0)/4, V_{l+1} <= 0.7·V_l — are held to the device; this file shows the margin each has in the
restatement, and tests/test_mlmc_host.py asks for 1.25x on both seeds.  Run on the CPU.

    python tests/golden/make_mlmc_exact.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import mlmc_cases as mc  # noqa: E402


def build():
    return dict(case=mc.MILD, steps=[mc.STEPS0 << l for l in range(len(mc.TRAJECTORIES))], trajectories=list(mc.TRAJECTORIES),
                seeds={str(s): mc.restate(s) for s in mc.RESTATED_SEEDS})


if __name__ == "__main__":
    with open(mc.GOLDEN, "w") as f:
        json.dump(build(), f, indent=1)
        f.write("\n")
    print(mc.GOLDEN)
