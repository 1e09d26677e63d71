"""k_flatten_wave's closed-form pass 2 against the host flattener, word for word: programs, plen,
nodes, status, JIT words and cost.

The shapes are the ones at which linking rows to their parents and summing a row's path to the root
could go wrong: an empty tree, a single leaf, a unary chain over every row (the deepest path), full
binary trees, left and right combs, constant subtrees that fold to one LDC, and slots that a
zero_mask turns constant in one program spec but not in another.  Arbitrary arrays bring operands
j >= i and rows with two parents (walked by one lane inside the same kernel; no second launch), one
of them an expansion longer than the kernel's LDS copy of the program.  P = 1 and 3 leave the last
wave without a partner program; NMAX 64 runs the register-mode sizing, NMAX 128 the LDS-data one."""
import ctypes
import functools

import numpy as np
import pytest

import multitreegp_amd as mt
from multitreegp_amd import _native as nat

from helpers import tree_from_expr

pytestmark = pytest.mark.gpu

OPS = [("+", None, 2, 0.3), ("-", None, 2, 0.1), ("*", None, 2, 0.3), ("/", None, 2, 0.1), ("sin", None, 1, 0.1),
       ("exp", None, 1, 0.1)]
VARS = ["x0", "x1", "x2", "x3", "x4", "x5"]
# zero masks: none, x0 + x1 (turns a subtree of `masked` constant), x2..x5
SPEC_SETS = {
    "one_per_tree": [(0, 6, 0), (1, 6, 0)],
    "two_on_one": [(0, 6, 0), (1, 6, 0b000011), (1, 6, 0b111100)],
    "three_on_one": [(0, 6, 0b000011), (0, 6, 0), (0, 6, 0b111100)],
}


def _full(depth, leaves):
    if depth == 0:
        return next(leaves)
    return ("+" if depth % 2 else "*", _full(depth - 1, leaves), _full(depth - 1, leaves))


def _leaves():
    k = 0
    while True:  # variables and coefficients in turn, never two coefficients side by side
        yield VARS[k % 6] if k % 3 else float(k % 7) - 2.5
        k += 1


def _shapes(lib, N):
    """[N, 4] trees, the smallest of each kind that fills N rows where the kind asks for it."""
    def chain(op, n):
        e = "x2"
        for _ in range(n):
            e = (op, e)
        return e

    def comb(left, n):
        e = "x0"
        for k in range(n):
            leaf = VARS[1 + k % 5] if k % 2 else 0.5 + k
            e = ("-", e, leaf) if left else ("/", leaf, e)
        return e

    depth = 6 if N == 64 else 7
    exprs = [
        "x3",                                       # a single leaf
        chain("sin", N - 1),                        # a unary chain over every row
        chain("exp", N - 1),
        _full(depth - 1, _leaves()),                # 2^depth - 1 rows
        comb(True, (N - 1) // 2),
        comb(False, (N - 1) // 2),
        ("*", ("+", ("sin", 1.5), ("*", 2.0, 0.25)), ("exp", ("-", 1.0, 3.0))),      # folds to one LDC
        ("+", ("*", ("sin", ("+", "x0", "x1")), ("-", "x1", 2.0)), ("/", "x4", ("exp", "x0"))),  # masked
        ("-", ("+", "x0", "x1"), ("*", ("+", "x0", 1.0), ("sin", ("*", "x2", "x5")))),
        3.25,                                       # a coefficient alone
        ("sin", ("+", ("*", "x5", "x4"), ("-", ("exp", "x3"), ("/", "x2", ("+", "x1", "x0"))))),
    ]
    trees = [np.zeros((N, 4), np.float32)]          # an empty tree
    trees[0][:, 1:3] = -1
    trees += [tree_from_expr(e, lib, N) for e in exprs]
    return trees


def _arbitrary(lib, N, rng):
    """Arrays no sampler makes: random rows, a root with one row as both operands, and doublings
    r_k = r_{k-1} + r_{k-1} whose program (fused 2^k - 1 words) outgrows the N + 8 words of the
    kernel's LDS copy while its unfused length still fits the slot."""
    out = []
    for _ in range(3):
        t = np.empty((N, 4), np.float32)
        t[:, 0] = rng.integers(-2, lib.n_funcs + 3, N) + (rng.random(N) < 0.1) * 0.5
        t[:, 1] = rng.integers(-N - 3, N + 3, N)
        t[:, 2] = rng.integers(-N - 3, N + 3, N)
        t[:, 3] = rng.standard_normal(N) * 3
        out.append(t)
    t = tree_from_expr(("*", ("sin", ("+", "x0", "x1")), "x2"), lib, N)
    t[N - 1, 2] = t[N - 1, 1]  # sin(x0 + x1) * sin(x0 + x1): one row, two parents
    out.append(t)
    k = 6 if N == 64 else 7
    t = np.zeros((N, 4), np.float32)
    t[:, 1:3] = -1
    t[0] = [lib.string_to_node["x0"], -1, -1, 0]
    t[1] = [lib.string_to_node["x1"], -1, -1, 0]
    t[2] = [lib.string_to_node["*"], 0, 1, 0]          # r_1
    for i in range(3, 2 + k):
        t[i] = [lib.string_to_node["+"], i - 1, i - 1, 0]  # r_2 .. r_k
    t[N - 1] = [lib.string_to_node["-"], 1 + k, k - 1, 0]  # r_k - r_{k-2}: 2^k + 2^(k-2) - 1 words
    out.append(t)
    t = t.copy()  # r_10: too long for the slot, and its operand stack too deep -> an error status
    for i in range(3, 12):
        t[i] = [lib.string_to_node["+"], i - 1, i - 1, 0]
    t[N - 1] = [lib.string_to_node["sin"], 11, -1, 0]
    out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def _case(N, mode, spec_key):
    """64 individuals of two trees each and the host flattener's result for every program."""
    lib = mt.NodeLibrary(OPS, [VARS], [2])
    rng = np.random.default_rng(7)
    trees = _shapes(lib, N) + _arbitrary(lib, N, rng)
    P = 64
    pop = np.stack([np.stack([trees[p % len(trees)], trees[(3 * p + 5) % len(trees)]]) for p in range(P)])
    specs = SPEC_SETS[spec_key]
    L = (2 * N + 8 + 3) // 4 * 4
    L_ = nat.load()
    libs = lib.native()
    host = np.zeros((P, len(specs), L, 2), np.int32)
    hn = np.zeros((P, len(specs)), np.int32)
    hw = np.zeros((P, len(specs)), np.int32)
    word = np.zeros(8192, np.uint32)
    for p in range(P):
        for j, (t, d, z) in enumerate(specs):
            hn[p, j] = L_.mtgp_flatten_tree_host(pop[p, t].ctypes.data, N, ctypes.byref(libs), d, z, L,
                                                 host[p, j].ctypes.data, None)
            w = L_.mtgp_jit_translate_host_ex(host[p, j].ctypes.data, L, word.ctypes.data, 8192, mode)
            hw[p, j] = w - 1 if w > 0 else w + 100
    for a in (pop, host, hn, hw):
        a.setflags(write=False)
    return lib, pop, specs, L, host, hn, hw


def _flatten_ex(pop, lib, specs, L, mode):
    import torch
    P, T, N, _ = pop.shape
    L_ = nat.load()
    dev = torch.device("cuda", 0)
    n_prog = len(specs)
    arr = (nat.MtgpProgramSpec * n_prog)()
    for i, (t, d, z) in enumerate(specs):
        arr[i].tree, arr[i].n_data, arr[i].zero_mask = t, d, z
    sp = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    pd = torch.from_numpy(np.array(pop, np.float32)).to(dev)  # (a copy: the shared reference is read-only)
    prog = torch.zeros((P * n_prog * L * 2 + 8,), dtype=torch.int32, device=dev)
    out = {k: torch.full(s, -77, dtype=torch.int32, device=dev) for k, s in
           (("plen", (P, n_prog)), ("nodes", (P,)), ("status", (P, n_prog)), ("jw", (P, n_prog)), ("jc", (P, n_prog)))}
    libs = lib.native()
    rc = L_.mtgp_flatten_ex(pd.data_ptr(), P, T, N, ctypes.byref(libs), sp.data_ptr(), n_prog, L, prog.data_ptr(),
                            out["plen"].data_ptr(), out["nodes"].data_ptr(), out["status"].data_ptr(),
                            out["jw"].data_ptr(), out["jc"].data_ptr(), mode, None)
    assert rc == nat.OK
    cost = None
    if mode == 0:  # the schedule weight of a finished program, by its own entry point
        cost = torch.empty((P, n_prog), dtype=torch.int32, device=dev)
        assert L_.mtgp_jit_cost(prog.data_ptr(), out["plen"].data_ptr(), P, n_prog, L, cost.data_ptr(), None) == 0
    torch.cuda.synchronize()
    progs = prog[: P * n_prog * L * 2].view(P, n_prog, L, 2).cpu().numpy()
    return progs, {k: v.cpu().numpy() for k, v in out.items()}, None if cost is None else cost.cpu().numpy()


@pytest.mark.parametrize("halves", ["1", "0", None])
@pytest.mark.parametrize("spec_key", list(SPEC_SETS))
@pytest.mark.parametrize("N,mode", [(64, 0), (128, 1)])
@pytest.mark.parametrize("P", [1, 3, 64])
def test_wave_flatten_matches_host_flattener(P, N, mode, spec_key, halves, monkeypatch):
    """Every forced packing (MTGP_FLAT_HALVES 1 / 0) and the default give the host's words."""
    if halves is None:
        monkeypatch.delenv("MTGP_FLAT_HALVES", raising=False)
    else:
        monkeypatch.setenv("MTGP_FLAT_HALVES", halves)
    lib, pop, specs, L, host, hn, hw = _case(N, mode, spec_key)
    pop = pop[:P]
    progs, out, cost = _flatten_ex(pop, lib, specs, L, mode)
    if P == 64:  # the population holds what the docstring promises
        assert (hn > N + 8).any() and (hn < 0).any() and (hn == 1).any()
    for p in range(P):
        assert out["nodes"][p] == int((pop[p, ..., 0] != 0).sum()), p
        for j in range(len(specs)):
            n = int(hn[p, j])
            assert out["plen"][p, j] == max(n, 0) and out["status"][p, j] == (0 if n > 0 else -n), (p, j, n)
            assert np.array_equal(progs[p, j, : max(n, 0) + 1], host[p, j, : max(n, 0) + 1]), (p, j)
            assert out["jw"][p, j] == hw[p, j], (p, j, out["jw"][p, j], hw[p, j])
    if cost is not None:
        assert np.array_equal(cost, out["jc"])
