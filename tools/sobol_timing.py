#!/usr/bin/env python3
"""hh_sobol_fill against hh_wiener_fill on 10^6 x 252 Heston increments, device-resident, in one sitting: the bridge and the
incremental construction, each the median of 9 timed calls between events on the context's stream after one untimed call
(which uploads the direction words and the bridge's table).  The floor of all three is one write of the buffer.  GPU box
only.  Writes what it prints to the file named on the command line (profiles/sobol_timing.txt)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hedgehog_jl_amd import _ffi

ctx = _ffi.get_context(0)
lib, h = ctx.lib, ctx.handle
n, steps = 1_000_000, 252
m = _ffi.make_model()
seeds = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
dst = torch.empty(lib.hh_replay_elems(n, steps, _ffi.HH_HESTON), dtype=torch.float64, device="cuda")
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
stream = torch.cuda.current_stream()
ctx.set_stream(stream.cuda_stream)
nbytes = 8 * dst.numel()


def sobol(construction):
    return lambda: lib.hh_sobol_fill(h, _ffi.HH_HESTON, m.rho, m.T, steps, n, 0, 20261020, 1, 1, construction, dst.data_ptr())


lines, times = [f"{n} points x {steps} steps, Heston (2 components): {nbytes / 1e9:.3f} GB written per fill; median of 9"], {}
for name, fn in (("hh_wiener_fill", lambda: lib.hh_wiener_fill(h, _ffi.HH_HESTON, m.rho, m.T, steps, n, seeds.data_ptr(), 1, dst.data_ptr())),
                 ("hh_sobol_fill bridge", sobol(_ffi.HH_SOBOL_BRIDGE)),
                 ("hh_sobol_fill incremental", sobol(_ffi.HH_SOBOL_INCREMENTAL)),
                 ("hh_wiener_fill again", lambda: lib.hh_wiener_fill(h, _ffi.HH_HESTON, m.rho, m.T, steps, n, seeds.data_ptr(), 1, dst.data_ptr()))):
    ctx.check(fn())
    torch.cuda.synchronize()
    ts = []
    for _ in range(9):
        ev[0].record(stream)
        ctx.check(fn())
        ev[1].record(stream)
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    times[name] = sorted(ts)[len(ts) // 2]
    lines.append(f"{name}: {times[name]:.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}), {nbytes / times[name] / 1e6:.0f} GB/s written, "
                 f"{n * steps / times[name] / 1e6:.1f} G point-steps/s")
base = 0.5 * (times["hh_wiener_fill"] + times["hh_wiener_fill again"])
for name in ("hh_sobol_fill bridge", "hh_sobol_fill incremental"):
    lines.append(f"{name} / hh_wiener_fill: {times[name] / base:.3f}")
print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
