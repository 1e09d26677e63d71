"""Pointwise regression: the fused kernel (PointwiseEvaluator -> k_pointwise) against the route it
replaces (DeviceEngine.eval_programs, then the fitness in torch), in one process, alternating.

P = 8192 candidates of one depth <= 10 tree over two inputs, M = 256, 4096 and 65536 points.  Two
timings per route and M, host clock around work that ends in a device synchronise, after warm-up:
  step: what a generation pays -- flatten included (the fused route also schedules and builds its JIT code);
  eval: the evaluation of an already flattened population (the fused route's code already built).
Prints one JSON line per M and writes them to --out (default profiles/pointwise/bench.json).

--scaled times linear scaling instead, "eval" only, three routes alternating: the scaled fused kernel
(k_pointwise<JIT, true>), the unscaled fused kernel of the same build, and the route scaling replaces --
the fused kernel's predictions [P, n_out, M] reduced by a float64 closed form in torch (default --out
profiles/pointwise/bench_scaled.json).

--n-var N: a table of N columns (default 2; more than 8 run in k_pointwise_wide, the data vector in LDS).
--wide-ab (N <= 8): "eval" only, two routes alternating -- the same population through k_pointwise_wide
(MTGP_PW_WIDE=1, LDS-data code) and through k_pointwise (register-data code) of the same build.
--append adds the lines to --out instead of replacing it (profiles/pointwise/bench_wide.json holds both)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multitreegp_amd as mt  # noqa: E402
from multitreegp_amd.engine import DeviceEngine  # noqa: E402
from multitreegp_amd.evaluators import _TreeOnly  # noqa: E402
from multitreegp_amd.sampling import sample_population  # noqa: E402

MAXF, PARSIMONY = 1e4, 0.01


def torch_fitness(pred, y_t, nodes):
    """The fitness on top of eval_programs' [P, n_out, M] predictions, as a user writes it in torch."""
    mean = ((pred - y_t[None]) ** 2).sum(1).mean(-1)
    mean = torch.where(torch.isfinite(mean), mean, torch.full_like(mean, MAXF)).clamp(0.0, MAXF)
    return mean + PARSIMONY * nodes.float()


def torch_scaled_fitness(pred, y_t, nodes):
    """Linear scaling on top of predictions, as a user writes it in torch: centred float64 moments."""
    f, y = pred.double(), y_t.double()[None]
    fc, yc = f - f.mean(-1, keepdim=True), y - y.mean(-1, keepdim=True)
    cff, cfy, cyy = (fc * fc).sum(-1), (fc * yc).sum(-1), (yc * yc).sum(-1)
    b = torch.where(cff > 2.0 ** -40 * (f * f).sum(-1), cfy / cff, torch.zeros_like(cff))
    mean = ((cyy - b * cfy).clamp_min(0.0).sum(1) / pred.shape[-1]).float()
    mean = torch.where(torch.isfinite(mean), mean, torch.full_like(mean, MAXF)).clamp(0.0, MAXF)
    return mean + PARSIMONY * nodes.float()


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=8192)
    ap.add_argument("--points", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scaled", action="store_true", help="time linear scaling (see the module docstring)")
    ap.add_argument("--n-var", type=int, default=2)
    ap.add_argument("--wide-ab", action="store_true", help="k_pointwise_wide against k_pointwise (see the module docstring)")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join("profiles", "pointwise", "bench_scaled.json" if a.scaled else
                                  "bench_wide.json" if a.wide_ab or a.n_var > 8 else "bench.json")
    assert torch.cuda.is_available(), "bench_pointwise needs the GPU"
    ops = [("+", None, 2, 0.5), ("-", None, 2, 0.1), ("*", None, 2, 0.5), ("/", None, 2, 0.1),
           ("sin", None, 1, 0.1), ("cos", None, 1, 0.1), ("exp", None, 1, 0.1)]
    nv = a.n_var
    assert nv >= 2 and not (a.wide_ab and (a.scaled or nv > 8)), "--wide-ab: unscaled, at most 8 columns"
    lib = mt.NodeLibrary(ops, [[f"x{k}" for k in range(nv)]], [1])
    ff = lambda **kw: mt.PointwiseEvaluator(MAXF, wide=nv > 8, **kw)  # noqa: E731
    pop = torch.from_numpy(sample_population(0, lib, a.P, 1, max_init_depth=10, max_nodes=63)[0]).cuda()
    rng = np.random.default_rng(1)
    lines = []
    for M in a.points:
        X = rng.uniform(-2, 2, size=(M, nv)).astype(np.float32)
        Y = (np.sin(X[:, :1]) * X[:, -1:]).astype(np.float32)
        new = DeviceEngine(ff(), lib, PARSIMONY, "cuda:0")
        new_eval = DeviceEngine(ff(), lib, PARSIMONY, "cuda:0")  # (keeps its built code)
        old = DeviceEngine(_TreeOnly(1, nv), lib, 0.0, "cuda:0")
        old.prepare_data(None)
        x_dev, y_t = torch.from_numpy(X).cuda(), torch.from_numpy(Y.T.copy()).cuda()
        fl_new, fl_old = new_eval.evaluate(pop, (X, Y))["_flat"], old.flatten(pop)

        def torch_step():
            fl = old.flatten(pop)
            return torch_fitness(old.eval_programs(fl, x_dev), y_t, fl.nodes)

        routes = {
            "fused_step": lambda: new.evaluate(pop, (X, Y), check=False)["fitness"],
            "torch_step": torch_step,
            "fused_eval": lambda: new_eval.evaluate(pop, (X, Y), flattened=fl_new, check=False)["fitness"],
            "torch_eval": lambda: torch_fitness(old.eval_programs(fl_old, x_dev), y_t, fl_old.nodes),
        }
        if a.scaled:
            sc = DeviceEngine(ff(linear_scaling=True), lib, PARSIMONY, "cuda:0")
            fl_sc = sc.evaluate(pop, (X, Y))["_flat"]

            def torch_scaled():
                res = new_eval.evaluate(pop, (X, Y), trajectories=True, flattened=fl_new, check=False)
                return torch_scaled_fitness(res["pred"], y_t, fl_new.nodes)

            routes = {"scaled_eval": lambda: sc.evaluate(pop, (X, Y), flattened=fl_sc, check=False)["fitness"],
                      "fused_eval": routes["fused_eval"], "torch_eval": torch_scaled}
        if a.wide_ab:  # the knob is read at every flatten, build and launch: one engine and one flattening per kernel
            wide_eng = DeviceEngine(ff(), lib, PARSIMONY, "cuda:0")

            def knob(on, fn):
                os.environ["MTGP_PW_WIDE"] = "1" if on else "0"
                return fn()

            fl_wide = knob(True, lambda: wide_eng.evaluate(pop, (X, Y))["_flat"])
            narrow = routes["fused_eval"]
            routes = {"wide_eval": lambda: knob(True, lambda: wide_eng.evaluate(pop, (X, Y), flattened=fl_wide,
                                                                                check=False)["fitness"]),
                      "torch_eval": lambda: knob(False, narrow)}  # (reported as narrow_eval)
        first = "scaled_eval" if a.scaled else "wide_eval" if a.wide_ab else "fused_eval"
        f_new, f_old = routes[first]().cpu().numpy(), routes["torch_eval"]().cpu().numpy()
        ms = {k: [] for k in routes}
        for r in range(a.warmup + a.reps):  # alternating: one call of every route per round
            for k, fn in routes.items():
                t = timed(fn, 1)
                if r >= a.warmup:
                    ms[k] += t
        line = dict(bench="pointwise", P=a.P, M=M, n_var=nv, n_out=1, reps=a.reps,
                    max_rel_diff=float(np.max(np.abs(f_new - f_old) / np.maximum(np.abs(f_old), 1e-30))),
                    **{f"{k}_ms": dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ms.items()})
        if a.scaled:
            med = {k: line[f"{k}_ms"]["median"] for k in routes}
            line["bench"] = "pointwise_scaled"
            line["ratio_scaled_over_unscaled"] = med["scaled_eval"] / med["fused_eval"]
            line["ratio_torch_over_scaled"] = med["torch_eval"] / med["scaled_eval"]
        if a.wide_ab:  # (the second route is k_pointwise: max_rel_diff must be 0)
            line["bench"], line["narrow_eval_ms"] = "pointwise_wide_ab", line.pop("torch_eval_ms")
            line["ratio_wide_over_narrow"] = line["wide_eval_ms"]["median"] / line["narrow_eval_ms"]["median"]
        for kind in () if a.scaled or a.wide_ab else ("step", "eval"):
            line[f"{kind}_ratio_torch_over_fused"] = line[f"torch_{kind}_ms"]["median"] / line[f"fused_{kind}_ms"]["median"]
        print(json.dumps(line), flush=True)
        lines.append(line)
        del routes, new, new_eval, old, fl_new, fl_old
        sc = fl_sc = None
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            lines = json.load(f) + lines
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
