#!/usr/bin/env python3
"""Two builds of libmtgp_host.so on the same parents, CPU only: bit-equality of the offspring and
the time of mtgp_evolve_populations, the libraries alternating call by call.

    scripts/evolve_ab.py --a PATH/libmtgp_host.so --b PATH/libmtgp_host.so [--threads 1,16] [--reps 7]

Setup per case (pop_size S, N rows, T trees): 2 populations, mixed operators (0.9 / 0.1 / 0),
migration on (every generation; --no-migration: never), elite 16, seed 77; the outputs are
preallocated and touched before timing.  One JSON line per (case, thread count)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import multitreegp_amd as mt  # noqa: E402
from multitreegp_amd import host  # noqa: E402
from helpers import CONTROL_OPS  # noqa: E402

CASES = {"S4096_N64_T3": (4096, 64, 3), "S1024_N256_T3": (1024, 256, 3), "S16384_N40_T3": (16384, 40, 3),
         "S65536_N64_T3": (65536, 64, 3), "c5_S2048_N128_T64": (2048, 128, 64)}
VARS = [["y1", "y2", "y3", "y4", "a1", "a2", "u"], ["a1", "a2"], ["y1", "y2"]]


def bind(path):
    lib = ctypes.CDLL(path)
    f32p, cfgp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(host.MtgpEvolveConfig)
    i32 = ctypes.c_int32
    lib.mtgp_evolve_populations.restype = ctypes.c_int
    lib.mtgp_evolve_populations.argtypes = [f32p, f32p, i32, i32, i32, i32, cfgp, ctypes.c_uint64, f32p]
    return lib


ap = argparse.ArgumentParser()
ap.add_argument("--a", required=True)
ap.add_argument("--b", required=True)
ap.add_argument("--threads", default="1,16")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--cases", default=",".join(CASES))
ap.add_argument("--no-migration", action="store_true", help="migration period 0 (no generation migrates)")
a = ap.parse_args()
libs = {"a": bind(a.a), "b": bind(a.b)}
f32p = ctypes.POINTER(ctypes.c_float)
for case in a.cases.split(","):
    S, N, T = CASES[case]
    lib = mt.NodeLibrary(CONTROL_OPS, [VARS[t % 3] for t in range(T)], [1] * T)
    tp = np.tile([0.6 * 0.4 ** i for i in range(7)], (2, 1))
    ev = host.HostEvolver(lib, N, 5, 1.0, 0 if a.no_migration else 1, 8, 7, 16, tp,
                          np.tile([0.9, 0.1, 0.0], (2, 1)), np.ones(2), 2)
    pops = ev.sample_population(S, seed=3)
    for g in range(2):  # parents with grown trees, not fresh samples
        pops = ev.evolve(pops, np.random.default_rng(g).random((2, S)).astype(np.float32), 5 + g, g).copy()
    fit = np.random.default_rng(4).random((2, S)).astype(np.float32)
    out = {k: np.zeros_like(pops) for k in libs}
    ev.cfg.current_generation = 0
    for nt in a.threads.split(","):
        os.environ["MTGP_HOST_THREADS"] = nt
        ms = {k: [] for k in libs}
        for rep in range(a.reps + 1):
            for k, l in libs.items():
                t0 = time.perf_counter()
                rc = l.mtgp_evolve_populations(pops.ctypes.data_as(f32p), fit.ctypes.data_as(f32p), 2, S, T, N,
                                               ctypes.byref(ev.cfg), 77, out[k].ctypes.data_as(f32p))
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == S, rc
                if rep:  # the first round warms up
                    ms[k].append(round(dt, 3))
        print(json.dumps({"case": case, "threads": int(nt), "migration": not a.no_migration,
                          "population_mb": round(pops.nbytes / 2**20, 1),
                          "bit_equal": bool(np.array_equal(out["a"].view(np.uint32), out["b"].view(np.uint32))),
                          "a_ms": ms["a"], "b_ms": ms["b"], "a_median": float(np.median(ms["a"])),
                          "b_median": float(np.median(ms["b"]))}), flush=True)
