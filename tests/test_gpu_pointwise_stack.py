"""PointwiseEvaluator on the GPU with deep operand stacks: 17 individuals (two workgroups of eight live waves and
one with a single live wave), every one a different + - * tree of 2 .. 128 leaves, so the waves of a workgroup run
different programs at different stack depths while both tile buffers are live.  In k_pointwise_wide the waves' stack
columns sit in dynamic LDS right behind the two tiles: a wave's stack reaching a neighbour's, or a tile, changes
bits here.  The schedule is not the identity (the sizes ascend with p, the schedule runs the longest first), so
order[q] against q indexing is checked against numpy, not against another kernel."""
import functools

import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from multitreegp_amd import _native as nat
from multitreegp_amd.engine import DeviceEngine
from helpers import bits_equal
from test_gpu_pointwise import fitness_ref, library, tree, value

pytestmark = pytest.mark.gpu
f32, MAXF = np.float32, 1e9  # (above every mean here: no fitness is clipped, all carry the sums' bits)
P, N_OUT, N = 17, 2, 256
LEAVES = (2, 3, 4, 5, 6, 8, 11, 16, 23, 32, 45, 64, 90, 100, 112, 120, 128)  # of output 0 of individual p
# Sethi-Ullman with fused leaf pairs: a leaf pair needs no slot, a node one more than its children when they need
# the same.  Depth d therefore takes 2^(d+1) leaves: 6 at the perfect tree on 128 leaves (255 rows), and depth 7
# would take 511 rows > MTGP_MAX_NODES.
PEAK_DEPTH = 6
_PUSH = ("LDCP", "LDVP", "SINVP", "COSVP")
_POP = ("ADDS", "SUBS", "RSUBS", "MULS", "DIVS", "RDIVS")


def deep_expr(p, out, n_var):
    """The balanced tree of individual p's output `out`: the operators follow a pattern in (p, position), the
    leaves read the variables through a permutation that depends on p; every 7th leaf is a constant."""
    n = LEAVES[p] if out == 0 else LEAVES[(7 * p + 3) % P]
    perm = np.random.default_rng(100 + p).permutation(n_var)

    def build(lo, hi):
        if hi - lo == 1:
            return f32(0.5 + 0.25 * (lo % 4)) if (lo + p) % 7 == 3 else f"x{perm[(lo + out) % n_var]}"
        mid = (lo + hi + 1) // 2
        return ("+-*"[(p + lo + hi + out) % 3], build(lo, mid), build(mid, hi))

    return build(0, n)


def wide_tile_points(n_var):
    """Points of a k_pointwise_wide tile: 64 T, T the largest of 4, 2, 1 within 64 KB of LDS."""
    return 64 * next(T for T in (4, 2, 1) if 2 * T * (n_var + N_OUT) * 256 + 16384 <= 65536 or T == 1)


@functools.lru_cache(maxsize=None)
def case(n_var):
    """-> (library, population, X, Y, float32 tree values [P, n_out, M], fitness_ref): one point past two tiles of
    the wide kernel (n_var > 8), M = 257 for the narrow one; computed once, read-only."""
    M = 2 * wide_tile_points(n_var) + 1 if n_var > 8 else 257
    rng = np.random.default_rng(11)
    X, Y = rng.normal(size=(M, n_var)).astype(f32), rng.normal(size=(M, N_OUT)).astype(f32)
    lib = library("+-*", n_var, N_OUT)
    exprs = [[deep_expr(p, d, n_var) for d in range(N_OUT)] for p in range(P)]
    pop = np.stack([np.stack([tree(lib, e, N) for e in ex]) for ex in exprs])
    want = np.stack([np.stack([value(e, X) for e in ex]) for ex in exprs])
    assert np.all(np.isfinite(want))  # (so that equal bits on two paths are equal numbers)
    ref = np.array([fitness_ref(w, Y, MAXF) for w in want])
    assert np.all(ref < f32(MAXF))
    for a in (pop, X, Y, want, ref):
        a.setflags(write=False)
    return lib, pop, X, Y, want, ref


def stack_depths(fl):
    """Peak operand-stack depth of every program [P, n_prog], from the decoded host copy of fl.prog."""
    raw, plen = fl.prog.cpu().numpy().view(np.uint32), fl.plen.cpu().numpy()
    out = np.zeros(plen.shape, int)
    for p, q in np.ndindex(*plen.shape):
        depth = 0
        for op, imm in raw[p, q, :plen[p, q]]:
            name = nat.decode_instr(int(op), int(imm))[0]
            depth += (name in _PUSH or name.startswith(("VCP_", "VVP_"))) - (name in _POP)
            assert depth >= 0
            out[p, q] = max(out[p, q], depth)
        assert depth == 0
    return out


def run(n_var, path, wide):
    lib, pop, X, Y, want, ref = case(n_var)
    eng = DeviceEngine(mt.PointwiseEvaluator(MAXF, wide=wide), lib, 0.0, "cuda:0", jit=path != "interpreter")
    if path == "small_buffer":  # a 16-byte code buffer: the kernel sees that the code does not fit and interprets
        arena = eng._arena
        eng._arena = lambda nbytes: (arena(nbytes)[0], 16)
    pt = torch.from_numpy(pop.copy()).cuda()
    eng.prepare_data((X, Y))  # (the evaluator learns n_var and n_out from the data)
    fl = eng.flatten(pt)
    # the programs, before anything evaluates them
    assert int(fl.status.max().item()) == 0
    depths = stack_depths(fl)
    assert depths.max() == depths[P - 1, 0] == PEAK_DEPTH < nat.STACK_MAX, depths
    assert len(set(depths.max(axis=1))) >= 3, depths
    assert int(fl.plen.min().item()) <= 2 and int(fl.plen.max().item()) >= 100  # a 3-row tree .. the 255-row tree
    assert int(fl.nodes.min().item()) <= 12 and int(fl.nodes.max().item()) >= 400  # rows of an individual's two trees
    order = eng.schedule(fl, 64).cpu().numpy()
    assert sorted(order) == list(range(P)) and not np.array_equal(order, np.arange(P)), order
    res = eng.evaluate(pt, (X, Y), trajectories=True, flattened=fl)
    torch.cuda.synchronize()
    if eng.use_jit:
        assert DeviceEngine.jit_ok(fl) == (path == "jit")
    return eng, res["fitness"].cpu().numpy(), res["pred"].cpu().numpy(), fl, order


@pytest.mark.parametrize("path", ["jit", "interpreter", "small_buffer"])
@pytest.mark.parametrize("n_var", [8, 17, 40, 64])  # k_pointwise, k_pointwise_wide with T = 4, 2, 1
def test_deep_stacks_bitexact_on_every_path(monkeypatch, n_var, path):
    """Every path equals the numpy float32 tree values and the spec's fitness in bits (all finite), hence each other."""
    monkeypatch.delenv("MTGP_PW_WIDE", raising=False)
    _, _, _, _, want, ref = case(n_var)
    eng, fit, pred, _, order = run(n_var, path, wide=n_var > 8)
    assert eng._pointwise_wide() == (n_var > 8)
    print(n_var, path, "schedule", order.tolist())
    assert bits_equal(pred, want), np.argwhere(pred.view(np.uint32) != want.view(np.uint32))[:8]
    assert bits_equal(fit, ref), (fit, ref)


@pytest.mark.parametrize("path", ["jit", "interpreter", "small_buffer"])
def test_deep_stacks_forced_wide_kernel_at_8_columns(monkeypatch, path):
    """MTGP_PW_WIDE=1: k_pointwise_wide (T = 4, two tiles at M = 257) gives the reference's, so k_pointwise's, bits."""
    monkeypatch.setenv("MTGP_PW_WIDE", "1")
    _, _, _, _, want, ref = case(8)
    eng, fit, pred, fl, _ = run(8, path, wide=False)
    assert eng._pointwise_wide() and eng._jit_mode() == nat.JIT_MODE_LDS
    assert path != "jit" or fl.jit[4].next == 0  # the wide kernel's code
    assert bits_equal(pred, want), np.argwhere(pred.view(np.uint32) != want.view(np.uint32))[:8]
    assert bits_equal(fit, ref), (fit, ref)
