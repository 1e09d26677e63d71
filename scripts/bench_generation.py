#!/usr/bin/env python
"""Wall time of whole generations (evaluate_population + evolve) at the C3 / C5 shapes of bench.py,
for evolve_backend "native" (host library: the population crosses PCIe every generation) and
"device" (csrc/mtgp_evolve.hip: it stays on the GPU).

Both backends start from bench.py's population (its workload builders, by import) and use the same
seeds, so -- the device step being the host step draw for draw -- they walk the same trajectory and
every generation compares like with like.  With --backend both (default) the two alternate
generation by generation in one process.  Each generation is timed on the host clock around a
device synchronise, split into evaluate and evolve.  Prints one JSON line per backend.

    python scripts/bench_generation.py --config c5 --warmup 5 --generations 20
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

DEPTH = {"c3": 10, "c5": 16}  # max_init_depth of bench.py's populations


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c3", choices=["c3", "c5"])
    ap.add_argument("--backend", default="both", choices=["native", "device", "both"])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--generations", type=int, default=20)
    ap.add_argument("--pop", type=int, default=None)
    ap.add_argument("--rollouts", type=int, default=None)
    ap.add_argument("--ode-steps", type=int, default=200)
    ap.add_argument("--solver", default="rk4", choices=["rk4", "dopri5"])
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    import bench
    import multitreegp_amd as mt
    bench.apply_config_defaults(args)
    env, lib, ff, data, pop = bench.setup_workload(args, 0)
    P, T, N = pop.shape[0], pop.shape[1], pop.shape[2]
    total = args.warmup + args.generations
    backends = ["native", "device"] if args.backend == "both" else [args.backend]
    runs = {}
    for b in backends:
        gp = mt.GeneticProgramming(total, P, ff, lib.operator_list, lib.variable_list, lib.layer_sizes,
                                   max_init_depth=DEPTH[args.config], max_nodes=N, migration_percentage=0.0,
                                   elite_percentage=0.125, device="cuda:0", verbose=False, evolve_backend=b)
        cur = torch.from_numpy(pop[None]).to("cuda:0") if b == "device" else pop[None]
        runs[b] = dict(gp=gp, pop=cur, evaluate=[], evolve=[])
    for g in range(total):
        for b in backends:  # alternate within the process
            r = runs[b]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit, cur = r["gp"].evaluate_population(r["pop"], data)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            r["pop"] = r["gp"].evolve(cur, fit, 1000 + g)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if g >= args.warmup:
                r["evaluate"].append((t1 - t0) * 1e3)
                r["evolve"].append((t2 - t1) * 1e3)
    for b in backends:
        r = runs[b]
        gen = np.add(r["evaluate"], r["evolve"])
        final = r["pop"].cpu().numpy() if b == "device" else r["pop"]
        print(json.dumps(dict(
            config=args.config, backend=b, pop=P, trees=T, max_nodes=N, rollouts=args.rollouts,
            warmup=args.warmup, generations=args.generations,
            generation_ms=dict(median=float(np.median(gen)), min=float(gen.min()), max=float(gen.max())),
            evaluate_ms=dict(median=float(np.median(r["evaluate"])), min=float(np.min(r["evaluate"])),
                             max=float(np.max(r["evaluate"]))),
            evolve_ms=dict(median=float(np.median(r["evolve"])), min=float(np.min(r["evolve"])),
                           max=float(np.max(r["evolve"]))),
            final_nodes=int(np.count_nonzero(final[..., 0])),
            host_evolve_threads=bench.host_evolve_threads())), flush=True)


if __name__ == "__main__":
    main()
