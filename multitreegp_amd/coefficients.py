"""Coefficient optimisation (gp.py:418-473).

Every 5th generation after generation 10 the reference takes the 50 best candidates and runs
``gradient_steps`` optimiser steps on their coefficients:

* ``epoch`` (gp.py:435-452): ``loss, grads = vmap(value_and_grad(partial_ff))(values, nodes,
  data)``, ``updates = optimiser.update(grads)``, ``values += updates``, emitting the PRE-update
  candidates and their loss;
* ``optimise`` (gp.py:454-473): the best loss over the epochs and the candidate it belongs to
  (first minimum).

Here the loss and gradient come from ``mtgp_sr_grad`` (the SR evaluator) and ``mtgp_ctl_grad``
(the dynamic and static control evaluators, every environment, state_size <= 16;
csrc/mtgp_grad.hip): forward-mode
dual numbers through the same RK4 / Euler solve as the evaluator, one GPU lane per (candidate,
parameter, rollout).  The parameters are the coefficient rows (``f == 1``) of every tree: the
host turns the rows of one chunk into variable rows that read data slots ``n_data + k`` (after
the evaluator's data vector), so the ordinary flattener produces the programs; other rows keep
their reference meaning.  The optimiser (optax's Adam restated in float32 numpy, ``adam``, or any
object with optax's init / update) runs on the host with one state per candidate, as the
reference's ``jax.vmap(self.optimiser.init)`` / ``jax.vmap(self.optimiser.update)`` do.  Given the
candidates as a CUDA tensor and the built-in ``Adam``, the same loop runs on the device instead
(``CoefficientOptimiser._optimise_device``, csrc/mtgp_optim.hip: this module's parameterise, Adam
and best-epoch choice restated in csrc/mtgp_optim_core.h, bit for bit).

Deviation (documented in DESIGN.md): JAX differentiates w.r.t. the whole value column, which
also reaches entries read through a reference to a LATER row (the "original column" case of
body_fun, gp.py:366-372).  Trees built by the reference's operators never read such an entry
(children sit below their parent, leaves ignore their index fields), so for them the gradients
agree; for arbitrary arrays only coefficient rows are optimised.

Adaptive solves (Dopri5 + PIDController): the gradient is the derivative of the discrete
solution along the step sequence the primal solve took -- step sizes, accept / reject decisions
and the NaN event carry no tangent.  That is diffrax's own rule under ``DirectAdjoint``: its
PIDController applies ``lax.stop_gradient`` to the initial step size (``init``) and to the
multiplicative step-size factor (``adapt_step_size``), so every step size has a zero tangent and
``jax.grad`` differentiates the discretised solution, not the ODE solution (diffrax is absent here:
restated from its published source, not executed).  Central differences of the float32 loss DO
move the step sizes, so they differ from it where a perturbation changes the accept / reject
sequence; over every finite, unclipped candidate (no smoothness filter, tests/test_coefficients.py)
the median relative difference is 7e-4, 75th percentile 3e-3, 90th 3e-2.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _native as nat


# ------------------------------------------------------------------------ optimiser
@dataclass
class AdamState:
    count: int
    mu: np.ndarray
    nu: np.ndarray


class Adam:
    """optax.adam(learning_rate, b1, b2, eps, eps_root) restated in float32 (optax
    scale_by_adam + scale_by_learning_rate): mu = (1-b1) g + b1 mu; nu = (1-b2) g^2 + b2 nu;
    mu_hat = mu / (1 - b1^t); nu_hat = nu / (1 - b2^t); update = -lr mu_hat / (sqrt(nu_hat +
    eps_root) + eps).  The reference's default (gp.py:79) is adam(0.001, 0.9, 0.999)."""

    def __init__(self, learning_rate: float = 0.001, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8,
                 eps_root: float = 0.0):
        self.learning_rate, self.b1, self.b2, self.eps, self.eps_root = learning_rate, b1, b2, eps, eps_root

    def init(self, params) -> AdamState:
        z = np.zeros(np.shape(params), np.float32)
        return AdamState(0, z, z.copy())

    def update(self, updates, state: AdamState, params=None):
        f = np.float32
        g = np.asarray(updates, np.float32)
        count = state.count + 1
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):  # float32 as jnp: inf / NaN, silently
            mu = f(1 - self.b1) * g + f(self.b1) * state.mu
            nu = f(1 - self.b2) * (g * g) + f(self.b2) * state.nu
            mu_hat = mu / (f(1) - f(self.b1) ** f(count))
            nu_hat = nu / (f(1) - f(self.b2) ** f(count))
            u = mu_hat / (np.sqrt(nu_hat + f(self.eps_root)) + f(self.eps))
        return (f(-self.learning_rate) * u).astype(np.float32), AdamState(count, mu, nu)

    def scalars(self, count: int) -> "nat.MtgpAdamScalars":
        """The float32 scalars of `update` at step `count` (the same numpy expressions), for
        mtgp_coef_adam_step: the device never evaluates a pow."""
        f = np.float32
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            return nat.MtgpAdamScalars(f(1 - self.b1), f(self.b1), f(1 - self.b2), f(self.b2),
                                       f(1) - f(self.b1) ** f(count), f(1) - f(self.b2) ** f(count),
                                       f(self.eps_root), f(self.eps), f(-self.learning_rate))


def adam(learning_rate: float = 0.001, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8,
         eps_root: float = 0.0) -> Adam:
    return Adam(learning_rate, b1, b2, eps, eps_root)


# ------------------------------------------------------------------- parameterise
def _f2i_sat(v: np.ndarray) -> np.ndarray:
    """f32 -> int32 truncation, saturating, NaN -> 0 (the flattener's int())."""
    v = np.asarray(v, np.float64)
    out = np.where(np.isnan(v), 0.0, np.clip(np.trunc(v), -2147483648.0, 2147483647.0))
    return out.astype(np.int64)


def coefficient_rows(candidates: np.ndarray) -> List[np.ndarray]:
    """Per candidate: the (tree, row) index pairs of its coefficient rows, row-major order."""
    return [np.argwhere(c[..., 0] == np.float32(1.0)) for c in candidates]


def parameterise(candidates: np.ndarray, rows: List[np.ndarray], lib, n_data: int, lo: int, hi: int):
    """Candidates with coefficient rows lo..hi-1 (per candidate) turned into variable rows that
    read data slots n_data + k.  Every other row keeps its meaning under the extended library:
    operator indices above the library are clamped as lax.switch does, variables past the data
    vector are pointed at its last slot (the flattener's clamp).
    -> (population [B, T, N, 4], theta [B, K], nparam [B], K, extended MtgpNodeLibrary)."""
    B = candidates.shape[0]
    pop = np.array(candidates, np.float32, copy=True)
    f = pop[..., 0]
    fi = _f2i_sat(f)
    coef = f == np.float32(1.0)
    top = lib.n_funcs - 1
    over = (~coef) & (fi > top)
    f[over] = np.float32(top)
    fi = np.where(over, top, fi)
    var_row = (~coef) & (fi >= lib.var_start) & (fi <= top) & (lib.fn_codes[np.clip(fi, 0, top)] == nat.FN_VAR)
    past = var_row & (fi - lib.var_start > n_data - 1)
    f[past] = np.float32(lib.var_start + n_data - 1)
    counts = np.array([max(0, min(hi, len(r)) - lo) for r in rows], np.int32)
    K = max(1, int(counts.max()) if B else 1)
    theta = np.zeros((B, K), np.float32)
    for b, r in enumerate(rows):
        for k in range(counts[b]):
            t, i = r[lo + k]
            theta[b, k] = pop[b, t, i, 3]
            pop[b, t, i, 0] = np.float32(lib.var_start + n_data + k)
    return pop, theta, counts, K, extended_library(lib, n_data, K)


def extended_library(lib, n_data: int, K: int):
    """The evaluator's node library followed by K parameter slots (variable rows reading data
    slots n_data .. n_data + K - 1) as an MtgpNodeLibrary."""
    n_funcs = max(lib.n_funcs, lib.var_start + n_data + K)
    if n_funcs > nat.MAX_FUNCS:
        raise ValueError(f"{n_funcs} node functions with {K} parameters > {nat.MAX_FUNCS}")
    fn = np.zeros(n_funcs, np.int8)
    fn[: lib.n_funcs] = lib.fn_codes
    fn[lib.var_start: n_funcs] = nat.FN_VAR
    return nat.node_library_struct(n_funcs, lib.var_start, fn)


def chunk_windows(counts, cap: int) -> List[Tuple[int, int]]:
    """(lo, K) of every chunk of at most `cap` coefficient rows per candidate, as loss_and_grad
    walks them: K = the most rows any candidate has in [lo, lo + cap), at least 1."""
    n_max = max([int(c) for c in counts] + [0])
    return [(lo, max([1] + [min(lo + cap, int(c)) - lo for c in counts])) for lo in range(0, max(n_max, 1), cap)]


# ----------------------------------------------------------------------- the loop
class CoefficientOptimiser:
    """GeneticProgramming.optimise on the GPU for one evaluator config (a DeviceEngine with
    size_parsinomy 0: the loss is the evaluator's fitness, gp.py:447)."""

    def __init__(self, engine, jit: Optional[bool] = None):
        self.check_evaluator(engine.ff)
        self.engine = engine
        # the control evaluators' programs as dual-number machine code (mtgp_ctl_grad_jit, ABI v19):
        # on with the engine's program JIT unless disabled here or by MTGP_GRAD_JIT=0
        self.use_jit = (engine.use_jit and os.environ.get("MTGP_GRAD_JIT", "1") != "0") if jit is None else bool(jit)
        self.last_jit_info = None  # device int32 [2] of the last call: [0] < 0 untranslatable, [1] bytes used

    @staticmethod
    def check_evaluator(ff):
        kind = getattr(ff, "solver_kind", "")
        if kind not in ("rk4", "euler", "dopri5"):
            raise NotImplementedError(f"coefficient optimisation: solver {kind!r} has no gradient kernels "
                                      "(implemented: euler, rk4, dopri5)")
        # (ABI v21: the dynamic evaluator's own limit; its constructor refuses more)
        if ff.model_id != nat.MODEL_SR and getattr(ff, "state_size", 0) > nat.GRAD_MAX_STATE:
            raise NotImplementedError(f"coefficient optimisation of the dynamic evaluator: state_size <= "
                                      f"{nat.GRAD_MAX_STATE}")

    @staticmethod
    def check_data(d: dict) -> None:
        """The data-dependent limits of the gradient kernels on a prepared data dict (the
        evaluator's `prepare`, host only), raised where the data is first seen
        (GeneticProgramming.evaluate_population at every generation with coefficient_optimisation,
        ADVICE r3), not at the first optimising generation (gp.py:418: generation 14): at most 64
        rollouts (one lane set per candidate).  (Since round 5 the general Acrobot cost mask -- ts off
        the one-pass grid, MtgpRollouts.fit_kof -- is differentiated too.)"""
        if d["R"] > 64:
            raise NotImplementedError("coefficient optimisation with more than 64 rollouts")

    def _grad_fn(self):
        eng = self.engine
        return eng.native.mtgp_sr_grad if eng.ff.model_id == nat.MODEL_SR else eng.native.mtgp_ctl_grad

    def param_cap(self, n_data: int) -> int:
        lib = self.engine.lib
        return max(1, min(nat.MAX_DATA - n_data, nat.MAX_FUNCS - lib.var_start - n_data))

    def loss_and_grad(self, candidates: np.ndarray, data, rows=None) -> Tuple[np.ndarray, List[np.ndarray]]:
        """loss [B] (the evaluator's fitness, no parsimony) and, per candidate, d loss / d value of
        each coefficient row in `rows` order."""
        eng = self.engine
        cands = np.ascontiguousarray(candidates, np.float32)
        B, T, N, _ = cands.shape
        rows = coefficient_rows(cands) if rows is None else rows
        g = _GradContext(self, data, N)
        dev = g.dev
        n_max = max([len(r) for r in rows] + [0])
        grads = [np.zeros(len(r), np.float32) for r in rows]
        loss = None
        for lo in range(0, max(n_max, 1), g.cap):
            pop, theta, nparam, K, libs = parameterise(cands, rows, eng.lib, g.n_data, lo, lo + g.cap)
            pop_dev = torch.from_numpy(pop).to(dev)
            prog, plen, nodes, status = g.program_buffers(B)
            g.flatten(pop_dev, libs, g.spec_dev(K), prog, plen, nodes, status)
            g.check_status(status)
            th = torch.from_numpy(theta).to(dev)
            npd = torch.from_numpy(nparam).to(dev)
            scratch = torch.empty((g.scratch_floats(B, K),), dtype=torch.float32, device=dev)
            lo_d = torch.empty((B,), dtype=torch.float32, device=dev)
            gr_d = torch.empty((B, K), dtype=torch.float32, device=dev)
            g.call(prog, B, th, npd, K, scratch, lo_d, gr_d, g.jit_buffers(B))
            gr = gr_d.cpu().numpy()
            if loss is None:
                loss = lo_d.cpu().numpy()
            for b in range(B):
                grads[b][lo: lo + nparam[b]] = gr[b, : nparam[b]]
        return loss, grads

    def optimise(self, candidates, data, n_epoch: int, optimiser=None):
        """gp.py:454-473 -> (fitness [B] = best loss over the epochs, candidates at that epoch).

        The result follows the input, as evaluate_population's does.  numpy in: the host loop,
        numpy out.  A CUDA tensor in: CUDA tensors out, and with the built-in optimiser (an `Adam`
        itself, not a subclass or another optax-style object) the whole loop runs on the device
        (`_optimise_device`: no candidate crosses to the host, the one read-back is the B
        coefficient counts that size the launches); any other optimiser, or MTGP_OPT_DEVICE=0,
        takes the host loop with the copies at its boundary."""
        opt = optimiser if optimiser is not None else adam()
        if isinstance(candidates, torch.Tensor) and candidates.is_cuda:
            if type(opt) is Adam and os.environ.get("MTGP_OPT_DEVICE", "1") != "0":
                return self._optimise_device(candidates, data, n_epoch, opt)
            fit, out = self.optimise(candidates.detach().cpu().numpy(), data, n_epoch, opt)
            dev = candidates.device
            return (torch.from_numpy(np.ascontiguousarray(fit, np.float32)).to(dev),
                    torch.from_numpy(np.ascontiguousarray(out, np.float32)).to(dev))
        cands = np.array(candidates, np.float32, copy=True)
        rows = coefficient_rows(cands)
        sizes = [len(r) for r in rows]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)

        def values(c):
            return np.concatenate([c[b][r[:, 0], r[:, 1], 3] for b, r in enumerate(rows)] + [np.zeros(0, np.float32)])

        vals = values(cands).astype(np.float32)
        # one optimiser state per candidate (gp.py:468 vmaps init, gp.py:448 vmaps update): an
        # optimiser with cross-element state (e.g. global-norm clipping) never couples candidates
        states = [opt.init(vals[offs[b]: offs[b + 1]]) for b in range(len(rows))]
        hist_c, hist_l = [], []
        for _ in range(int(n_epoch)):
            loss, grads = self.loss_and_grad(cands, data, rows)
            hist_c.append(cands.copy())
            hist_l.append(loss)
            for b, r in enumerate(rows):
                v = vals[offs[b]: offs[b + 1]]
                upd, states[b] = opt.update(np.asarray(grads[b], np.float32), states[b], v)
                vals[offs[b]: offs[b + 1]] = (v + np.asarray(upd, np.float32)).astype(np.float32)
                cands[b][r[:, 0], r[:, 1], 3] = vals[offs[b]: offs[b + 1]]
        L = np.stack(hist_l)
        best = np.argmin(L, axis=0)
        out = np.stack([hist_c[e][b] for b, e in enumerate(best)]) if len(best) else cands[:0]
        return L.min(axis=0), out

    def _optimise_device(self, candidates: torch.Tensor, data, n_epoch: int, opt: Adam):
        """`optimise` with the candidates on the GPU throughout (csrc/mtgp_optim.hip, DESIGN.md
        "Device optimise"), the host loop's result bit for bit.  The coefficient rows never change
        during the loop, only their values, and the gradient entry points take the values as theta:
        with one chunk (every candidate has at most param_cap coefficient rows, the common case)
        the candidates are parameterised and flattened once and an epoch is one gradient call and
        one fused track + Adam step, nothing read back.  With several chunks the other chunks'
        coefficients are literals in the programs, so parameterise + flatten repeat per epoch, on
        the device.  Host reads: the B coefficient counts (they size K, the program specs and the
        node library) and the flatten status, once each."""
        if int(n_epoch) < 1:
            raise ValueError("optimise needs at least one epoch")
        eng = self.engine
        dev = eng.device
        lib = eng.native
        cands = candidates.detach().to(dev, torch.float32).contiguous()
        if cands.data_ptr() % 16:
            cands = cands.clone()
        B, T, N, four = cands.shape
        if four != 4:
            raise ValueError("candidate rows must have 4 columns [f, a, b, value]")
        fit = torch.empty((B,), dtype=torch.float32, device=dev)
        if B == 0:
            return fit, cands.clone()
        g = _GradContext(self, data, N)
        stream = g.stream

        def ok(rc, name):
            if rc != nat.OK:
                raise RuntimeError(f"{name} failed: {rc}")

        work = cands.clone()  # the value column moves with every epoch; `cands` stays the input
        rowidx = torch.empty((B, T * N), dtype=torch.int32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        ok(lib.mtgp_coef_index(work.data_ptr(), B, T, N, rowidx.data_ptr(), count.data_ptr(), stream), "mtgp_coef_index")
        counts = count.cpu().numpy()  # the one read-back the sizing needs
        windows = chunk_windows(counts, g.cap)
        single = len(windows) == 1
        M = max(1, int(counts.max()))
        k_max = max(K for _, K in windows)
        # every buffer of the call: programs, scratch and code are shared by the chunks (stream
        # order), theta / nparam / gradient are per chunk (all chunks see the pre-update values)
        pop = torch.empty_like(work)
        prog, plen, nodes, status = g.program_buffers(B)
        scratch = torch.empty((g.scratch_floats(B, k_max),), dtype=torch.float32, device=dev)
        jit = g.jit_buffers(B)
        mu = torch.empty((B, M), dtype=torch.float32, device=dev)
        nu, best_vals = torch.empty_like(mu), torch.empty_like(mu)
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        loss_rest = torch.empty_like(loss)  # the other chunks' (equal) loss: the first chunk's counts
        worst = torch.zeros((), dtype=torch.int32, device=dev)
        chunks = []
        for lo, K in windows:
            chunks.append(dict(lo=lo, K=K, libs=extended_library(eng.lib, g.n_data, K), spec=g.spec_dev(K),
                               theta=torch.empty((B, K), dtype=torch.float32, device=dev),
                               nparam=torch.empty((B,), dtype=torch.int32, device=dev),
                               grad=torch.empty((B, K), dtype=torch.float32, device=dev)))
        base_lib = eng.lib.native()
        out = torch.empty_like(work)

        def programs(c):
            ok(lib.mtgp_coef_parameterise(work.data_ptr(), B, T, N, ctypes.byref(base_lib), g.n_data, c["lo"], c["K"],
                                          pop.data_ptr(), c["theta"].data_ptr(), c["nparam"].data_ptr(), stream),
               "mtgp_coef_parameterise")
            g.flatten(pop, c["libs"], c["spec"], prog, plen, nodes, status)

        for epoch in range(int(n_epoch)):
            for i, c in enumerate(chunks):
                if epoch == 0 or not single:
                    programs(c)
                    if epoch == 0:
                        g.check_status(status)
                    else:
                        torch.maximum(worst, status.max(), out=worst)
                g.call(prog, B, c["theta"], c["nparam"], c["K"], scratch, loss if i == 0 else loss_rest, c["grad"], jit)
            s = opt.scalars(epoch + 1)
            for i, c in enumerate(chunks):
                ok(lib.mtgp_coef_adam_step(work.data_ptr(), B, T, N, rowidx.data_ptr(), count.data_ptr(), c["lo"],
                                           c["K"], M, c["grad"].data_ptr(), loss.data_ptr(), ctypes.byref(s),
                                           int(epoch == 0), int(i == len(chunks) - 1), mu.data_ptr(), nu.data_ptr(),
                                           best_vals.data_ptr(), fit.data_ptr(),
                                           c["theta"].data_ptr() if single else None, stream), "mtgp_coef_adam_step")
        ok(lib.mtgp_coef_scatter(cands.data_ptr(), B, T, N, M, best_vals.data_ptr(), out.data_ptr(), stream),
           "mtgp_coef_scatter")
        if not single and int(n_epoch) > 1:
            g.check_status(worst)
        return fit, out


class _GradContext:
    """What one gradient call needs of the engine and the data, shared by the host loop
    (loss_and_grad) and the device loop (_optimise_device): the model and rollout structs, the
    program specs with K parameter slots, the flatten of a parameterised population and the call of
    the gradient entry point itself (interpreter or dual-number code)."""

    def __init__(self, opt: CoefficientOptimiser, data, N: int):
        eng = opt.engine
        self.opt, self.eng = opt, eng
        self.d = d = eng.prepare_data(data)
        opt.check_data(d)
        self.n_data = n_data = eng.ff.n_data()
        self.specs, _ = eng._specs()
        self.n_prog = len(self.specs)
        self.cap = opt.param_cap(n_data)
        self.dev = eng.device
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.m = eng.model_struct(d)
        self.ro = eng.rollouts_struct(d)
        self.R = d["R"]
        self.L = eng.program_stride(N)
        # (the general Acrobot mask keeps every lane's cost prefixes behind the partials, mtgp.h)
        self.hist = d["n_save"] if d.get("fit_kof") is not None else 0
        sr = eng.ff.model_id == nat.MODEL_SR
        self.grad_fn = opt._grad_fn()
        self.jit_fn = eng.native.mtgp_sr_grad_jit if sr else eng.native.mtgp_ctl_grad_jit
        # dual-number code: the register-data kernels only (SR with n_var <= 4, control with
        # state_size <= 3); wide dynamic states interpret from LDS columns (mtgp.h ABI v21)
        self.wide = not sr and getattr(eng.ff, "state_size", 0) > 3
        self.use_code = opt.use_jit and not self.wide and (not sr or n_data <= 4)

    def spec_dev(self, K: int) -> torch.Tensor:
        spec_arr = (nat.MtgpProgramSpec * len(self.specs))()
        for i, sp in enumerate(self.specs):  # the reference's data vector + K parameter slots (no slot gap)
            spec_arr[i].tree, spec_arr[i].n_data, spec_arr[i].zero_mask = sp[0], sp[1] + K, sp[2]
        return torch.frombuffer(bytearray(bytes(spec_arr)), dtype=torch.uint8).to(self.dev)

    def program_buffers(self, B: int):
        dev, n_prog = self.dev, self.n_prog
        prog = torch.empty((B * n_prog * self.L * 2 + 8,), dtype=torch.int32, device=dev)
        plen = torch.empty((B, n_prog), dtype=torch.int32, device=dev)
        nodes = torch.empty((B,), dtype=torch.int32, device=dev)
        status = torch.empty((B, n_prog), dtype=torch.int32, device=dev)
        return prog, plen, nodes, status

    def flatten(self, pop_dev: torch.Tensor, libs, spec_dev, prog, plen, nodes, status) -> None:
        B, T, N, _ = pop_dev.shape
        rc = self.eng.native.mtgp_flatten(pop_dev.data_ptr(), B, T, N, ctypes.byref(libs), spec_dev.data_ptr(),
                                          self.n_prog, self.L, prog.data_ptr(), plen.data_ptr(), nodes.data_ptr(),
                                          status.data_ptr(), self.stream)
        if rc != nat.OK:
            raise RuntimeError(f"mtgp_flatten (parameterised) failed: {rc}")

    @staticmethod
    def check_status(status: torch.Tensor) -> None:
        worst = int(status.max().item()) if status.numel() else 0
        if worst != 0:
            raise ValueError(f"parameterised candidate does not flatten (status {worst})")

    def scratch_floats(self, B: int, K: int) -> int:
        return B * K * self.R * 2 * (1 + self.hist)

    def jit_buffers(self, B: int):
        """(MtgpGradJit, offsets, info) when the call runs dual-number code, else None."""
        if self.wide:
            self.opt.last_jit_info = None
        if not self.use_code:
            return None
        code, nbytes = self.eng.grad_code_buffer(nat.grad_jit_bytes(B, self.n_prog, self.L))
        offs = torch.empty((B * self.n_prog + 1,), dtype=torch.int32, device=self.dev)
        info = torch.empty((2,), dtype=torch.int32, device=self.dev)
        return nat.MtgpGradJit(code, nbytes, offs.data_ptr(), info.data_ptr()), offs, info

    def call(self, prog, B: int, th, npd, K: int, scratch, loss_out, grad_out, jit) -> None:
        """mtgp_sr_grad / mtgp_ctl_grad (jit None) or their _jit forms on the current stream."""
        args = (ctypes.byref(self.m), prog.data_ptr(), self.n_prog, self.L, B, th.data_ptr(), npd.data_ptr(), K,
                ctypes.byref(self.ro), scratch.data_ptr(), loss_out.data_ptr(), grad_out.data_ptr())
        if jit is not None:
            called = self.jit_fn
            rc = called(*args, ctypes.byref(jit[0]), self.stream)
            self.opt.last_jit_info = jit[2]
        else:
            called = self.grad_fn
            rc = called(*args, self.stream)
        if rc != nat.OK:
            raise RuntimeError(f"{called.__name__} rejected the configuration (code {rc})")
