"""Time CoefficientOptimiser.loss_and_grad for dynamic Acrobot policies with wide hidden states
(state_size 4, 8, 16: k_ctl_grad_wide, LDS columns) against state_size 3 through the register
kernel's interpreter (jit=False), on the reference's optimising shape: 50 candidates (gp.py:418),
16 rollouts, 200 RK4 steps.  HIP events around the call, one warm-up per case, the cases
interleaved over the repeats.  Each case also runs with a single RK4 step, so that the part of the
call that is not the solve (parameterise, flatten, copies, launch) can be taken off; the
per-(lane x step x tree) cost is (t_200 - t_1) / (lanes * 199 * (state_size + 1)).
One JSON line per case, then the wide / narrow ratios."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from helpers import dynamic_setup  # noqa: E402
from multitreegp_amd import coefficients as co  # noqa: E402
from multitreegp_amd.engine import DeviceEngine  # noqa: E402

REPS = 20


def case(state_size, n_steps):
    env, lib, ff, data, pop = dynamic_setup(P=50, R=16, n_steps=n_steps, depth=6, N=40, seed=3,
                                            state_size=state_size)
    eng = DeviceEngine(ff, lib, 0.0, torch.device("cuda", 0))
    opt = co.CoefficientOptimiser(eng, jit=False)
    rows = co.coefficient_rows(pop)
    lanes = 16 * int(sum(max(len(r), 1) for r in rows))  # one per (candidate, coefficient, rollout)
    return dict(state_size=state_size, n_steps=n_steps, opt=opt, data=data, pop=pop, lanes=lanes, ms=[])


def main():
    cases = [case(ss, n) for ss in (3, 4, 8, 16) for n in (200, 1)]
    for c in cases:  # warm-up: data upload, code object load, the kernel's LDS limit
        c["opt"].loss_and_grad(c["pop"], c["data"])
    torch.cuda.synchronize()
    for _ in range(REPS):
        for c in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c["opt"].loss_and_grad(c["pop"], c["data"])
            e1.record()
            e1.synchronize()
            c["ms"].append(e0.elapsed_time(e1))
    med = {}
    for c in cases:
        med[(c["state_size"], c["n_steps"])] = m = float(np.median(c["ms"]))
        print(json.dumps({"state_size": c["state_size"], "rk4_steps": c["n_steps"], "candidates": 50, "rollouts": 16,
                          "lanes": c["lanes"], "ms_median": m, "ms_min": float(np.min(c["ms"])),
                          "ms_max": float(np.max(c["ms"])), "reps": REPS}), flush=True)
    lanes = {c["state_size"]: c["lanes"] for c in cases}

    def unit(ss):  # ns per (lane x step x tree)
        return 1e6 * (med[(ss, 200)] - med[(ss, 1)]) / (lanes[ss] * 199 * (ss + 1))

    for ss in (4, 8, 16):
        print(json.dumps({"state_size": ss, "ns_per_lane_step_tree": unit(ss), "narrow_ns_per_lane_step_tree": unit(3),
                          "ratio_wide_over_narrow": unit(ss) / unit(3)}), flush=True)


if __name__ == "__main__":
    main()
