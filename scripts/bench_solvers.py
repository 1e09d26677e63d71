#!/usr/bin/env python3
"""Time the C3 shape (bench.py's workload: DynamicPolicy Acrobot, pop 8192 x 32 rollouts, dt0 0.05 x
200 steps, trajectories on) once per fixed-step solver, all in one process on one GPU, and write the
result under profiles/erk/.  A step is one evaluate pass (flatten + schedule + JIT + kernel), as in
bench.py; kernel_ms is the evaluator launches' own HIP-event time.  The RHS-evaluation count per
step is the stage count (Bosh3: 3, its fourth stage is the next step's first).

    python scripts/bench_solvers.py [--steps 30] [--warmup 5] [--out profiles/erk/bench_solvers.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# solver -> RHS evaluations per step
SOLVERS = {"euler": 1, "heun": 2, "midpoint": 2, "ralston": 2, "bosh3": 3, "rk4": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pop", type=int, default=None)
    ap.add_argument("--rollouts", type=int, default=None)
    ap.add_argument("--solvers", default=",".join(SOLVERS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "erk", "bench_solvers.json"))
    a = ap.parse_args()
    import torch
    import bench
    import multitreegp_amd as mt
    from multitreegp_amd import _native as nat
    from multitreegp_amd.engine import DeviceEngine

    ns = bench.apply_config_defaults(argparse.Namespace(pop=a.pop, rollouts=a.rollouts, ode_steps=200, config="c3",
                                                        solver="rk4", obs_noise=0.0))
    env, lib, _, data, pop = bench.setup_workload(ns, 0)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pop_dev = torch.from_numpy(pop).to(dev)
    native = nat.load()
    native.mtgp_set_timing(1)
    rows = []
    for name in a.solvers.split(","):
        ff = mt.DynamicEvaluator(env, 2, 0.05, solver=name, max_steps=1000)
        eng = DeviceEngine(ff, lib, 0.0, dev)
        d = eng.prepare_data(data)
        res = eng.evaluate(pop_dev, data, trajectories=True, check=False)
        eng.check_status(res["_flat"])
        for _ in range(a.warmup):
            eng.evaluate(pop_dev, data, trajectories=True, check=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            res = eng.evaluate(pop_dev, data, trajectories=True, check=False)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        n = min(a.steps, 1024)
        hist = (ctypes.c_float * n)()
        if native.mtgp_kernel_ms_history(hist, n) != n:
            raise RuntimeError("kernel timing history is short")
        units = pop.shape[0] * d["R"] * d["n_steps"]
        fit = res["fitness"].cpu().numpy()
        rows.append({"solver": name, "rhs_per_step": SOLVERS[name], "ode_steps": d["n_steps"], "ms_per_step": ms,
                     "kernel_ms": float(np.mean(list(hist))), "kernel_ms_min": float(np.min(list(hist))),
                     "value": units / (ms / 1e3), "unit": "ODE-steps/s",
                     "finite_fitness_frac": float(np.mean(np.isfinite(fit)))})
        print(json.dumps(rows[-1]), flush=True)
    rk4 = next((r for r in rows if r["solver"] == "rk4"), None)
    for r in rows:
        r["kernel_ms_over_rk4"] = None if rk4 is None else r["kernel_ms"] / rk4["kernel_ms"]
    out = {"workload": f"C3 DynamicPolicy Acrobot: pop {pop.shape[0]} x {ns.rollouts} rollouts, 3 trees, dt0 0.05, "
                       f"S=201, trajectories on; {a.steps} timed steps after {a.warmup} warm-up, one process",
           "device": torch.cuda.get_device_name(dev), "build": nat.build_info().get("sources_sha256"), "solvers": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
