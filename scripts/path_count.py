#!/usr/bin/env python3
"""How often the C3 evaluator's stages leave a fast path, and for whom: diagnostic library built with
MTGP_AB_PATHCOUNT=1 (scripts/build_ab.py pathcount=MTGP_AB_PATHCOUNT=1[,MTGP_DEAD_ZERO=0]).

Counts wave-stages of the dynamic JIT loop that take the general branch of ctl_obs_apply, the slow
branch of mtgp_fmod_2pi (either wrap), the drift's slow trig reduction (trig_args_small) and its two
div_safe fallbacks, each split into "some live lane needed it" and "only ended / inactive lanes did",
next to the number of wave-stages and of those run by a wave that holds an ended or inactive lane."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multitreegp_amd import _native as nat  # noqa: E402
from multitreegp_amd.engine import DeviceEngine  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c3")
ap.add_argument("--lib", default="pathcount", help="library name under multitreegp_amd/lib/abrun/")
args = ap.parse_args()
ns = argparse.Namespace(pop=None, rollouts=None, ode_steps=200, config=args.config, solver="rk4", obs_noise=0.0)
ns = bench.apply_config_defaults(ns)
env, lib, ff, data, pop = bench.setup_workload(ns, 0)
path = os.path.join(ROOT, "multitreegp_amd", "lib", "abrun", f"libmtgp_hip_{args.lib}.so")
native = nat.load(path)
eng = DeviceEngine(ff, lib, 0.0, "cuda:0", native=native)
f = native.mtgp_ab_path_count
cnt = (ctypes.c_ulonglong * 12)()
pd = torch.from_numpy(pop).cuda()
eng.evaluate(pd, data, trajectories=True)
torch.cuda.synchronize()
f(cnt)  # (reads and clears: the first evaluation is dropped)
eng.evaluate(pd, data, trajectories=True)
torch.cuda.synchronize()
f(cnt)
names = ["obs_general", "fmod_slow", "trig_slow", "div_num_slow", "div_n1_slow"]
out = {"lib": args.lib, "waves": (ns.pop * ns.rollouts + 63) // 64, "wave_stages": cnt[10],
       "wave_stages_with_dead_lane": cnt[11]}
for i, n in enumerate(names):
    out[n] = {"live_needed": cnt[2 * i], "dead_only": cnt[2 * i + 1]}
print(json.dumps(out))
