#!/usr/bin/env python
"""Wall time of one optimising generation (evaluate_population at generation 14 with
coefficient_optimisation: evaluate, top 50, `gradient_steps` optimiser epochs, scatter) on a
population that lies on the GPU, for the two loops of CoefficientOptimiser.optimise:

    host    MTGP_OPT_DEVICE=0: the 50 best cross to the host, every epoch re-parameterises in
            Python, uploads, flattens, downloads loss and gradient and runs Adam in numpy
    device  the default: index, parameterise, gradient, fused track + Adam and scatter on the GPU
            (csrc/mtgp_optim.hip)

The legs alternate call by call in one process after warm-up, each timed on the host clock around
a device synchronise; `optimise_ms` is the part spent inside optimise.  --legs host,host runs the
host loop against itself (the A/A spread).  Prints one JSON line per leg.

    python scripts/bench_optimise.py --config c3 --warmup 3 --repeats 15
    python scripts/bench_optimise.py --config sr --legs host,host

--trace-epochs N runs nothing but one optimise call of 50 candidates with n_epoch N (for a
memory-copy trace of that call: its device-to-host copies must not depend on N).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(args):
    """(ff, lib, data, pop, max_init_depth): bench.py's C3 workload, or an SR shape (Van der Pol,
    2 variables, pop 4096, 8 rollouts, 50 save points, max_nodes 30)."""
    import bench
    import multitreegp_amd as mt
    from multitreegp_amd.sampling import sample_population
    if args.config == "c3":
        args.solver, args.ode_steps = "rk4", 200
        bench.apply_config_defaults(args)
        env, lib, ff, data, pop = bench.setup_workload(args, 0)
        return ff, lib, data, pop, 10
    args.pop, args.rollouts = args.pop or 4096, args.rollouts or 8
    env = mt.VanDerPolOscillator(0, 0)
    lib = mt.NodeLibrary([("+", None, 2, 0.5), ("-", None, 2, 0.1), ("*", None, 2, 0.5), ("/", None, 2, 0.1)],
                         [["x0", "x1"]], [2])
    ff = mt.SREvaluator(solver=mt.RK4(), dt0=0.05)
    x0 = env.sample_init_states(args.rollouts, np.random.default_rng(1))
    ts = (np.arange(50, dtype=np.float32) * np.float32(0.2)).astype(np.float32)
    data = (x0, ts, mt.ground_truth(env, x0, ts), np.zeros((args.rollouts, 2), np.uint32))
    pop = sample_population(4000, lib, args.pop, 1, max_init_depth=5, max_nodes=30)[0]
    return ff, lib, data, pop, 5


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c3", choices=["c3", "sr"])
    ap.add_argument("--legs", default="host,device", help="comma-separated: host / device, alternated in this order")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--gradient-steps", type=int, default=10)
    ap.add_argument("--pop", type=int, default=None)
    ap.add_argument("--rollouts", type=int, default=None)
    ap.add_argument("--trace-epochs", type=int, default=0)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    import multitreegp_amd as mt
    from multitreegp_amd import coefficients as co
    ff, lib, data, pop, depth = workload(args)
    P, T, N = pop.shape[0], pop.shape[1], pop.shape[2]

    if args.trace_epochs:
        from multitreegp_amd.engine import DeviceEngine
        opt = co.CoefficientOptimiser(DeviceEngine(ff, lib, 0.0, torch.device("cuda", 0)))
        cands = torch.from_numpy(pop[:50]).cuda()
        opt.engine.prepare_data(data)
        torch.cuda.synchronize()
        fit, out = opt.optimise(cands, data, args.trace_epochs)
        torch.cuda.synchronize()
        print(json.dumps(dict(config=args.config, trace_epochs=args.trace_epochs, candidates=int(cands.shape[0]),
                              device_loop=os.environ.get("MTGP_OPT_DEVICE", "1") != "0")), flush=True)
        return

    legs = args.legs.split(",")
    assert all(leg in ("host", "device") for leg in legs)
    gp = mt.GeneticProgramming(20, P, ff, lib.operator_list, lib.variable_list, lib.layer_sizes, max_init_depth=depth,
                               max_nodes=N, migration_percentage=0.0, elite_percentage=0.125, device="cuda:0",
                               verbose=False, evolve_backend="device",
                               coefficient_optimisation=True, gradient_steps=args.gradient_steps)
    inner = gp._optimise_shard
    spent = []

    def timed_optimise(cands, d):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = inner(cands, d)
        torch.cuda.synchronize()
        spent.append((time.perf_counter() - t0) * 1e3)
        return res

    gp._optimise_shard = timed_optimise
    pop_dev = torch.from_numpy(pop[None]).to("cuda:0")
    times = [dict(generation=[], optimise=[]) for _ in legs]
    checks = [None] * len(legs)
    for rep in range(args.warmup + args.repeats):
        for i, leg in enumerate(legs):  # alternate within the process
            if leg == "host":
                os.environ["MTGP_OPT_DEVICE"] = "0"
            else:
                os.environ.pop("MTGP_OPT_DEVICE", None)
            gp.current_generation = 14
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit, newpop = gp.evaluate_population(pop_dev, data)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep >= args.warmup:
                times[i]["generation"].append((t1 - t0) * 1e3)
                times[i]["optimise"].append(spent[-1])
            checks[i] = float(fit.double().sum().item())
    os.environ.pop("MTGP_OPT_DEVICE", None)

    def stats(x):
        return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))

    for i, leg in enumerate(legs):
        print(json.dumps(dict(config=args.config, leg=leg, leg_index=i, pop=P, trees=T, max_nodes=N,
                              rollouts=args.rollouts, candidates=min(50, P), gradient_steps=args.gradient_steps,
                              warmup=args.warmup, repeats=args.repeats, generation_ms=stats(times[i]["generation"]),
                              optimise_ms=stats(times[i]["optimise"]), fitness_sum=checks[i])), flush=True)


if __name__ == "__main__":
    main()
