"""The inputs of tests/test_gpu_pointwise_spans.py, and a guard on them that needs no GPU: on those
tables the reference's pairwise span tree and a left fold of the same span sums differ in bits, so
the bit comparison of the span tests cannot pass on a kernel that combines the spans in another
order.  (At W = 3 and W = 5 the two orders coincide -- zero padding makes the tree a left fold --
and the dyadic tables of the other tests round too rarely to tell.)  A condition on the inputs,
computed from the reference alone."""
import functools

import numpy as np
import pytest

from test_gpu_pointwise import exact_exprs, fitness_ref, value

f32 = np.float32
SPAN_SEED, SPAN_P, SPAN_N_OUT = 15, 9, 3  # (a seed picked for the guard below: 4, 9, 3 and 4 of 9 differ)
SPAN_M = (8193, 20481, 24577)  # W = 3, 6, 7: a one-point last span, zeros up to 4, 8 and 8 spans


def span_table(M, n_var):
    """float32 normal X [M, n_var], Y [M, SPAN_N_OUT]."""
    rng = np.random.default_rng(SPAN_SEED)
    return rng.normal(size=(M, n_var)).astype(f32), rng.normal(size=(M, SPAN_N_OUT)).astype(f32)


@functools.lru_cache(maxsize=None)
def span_case(M, n_var):
    """-> (X, Y, expressions, their float32 values [P, n_out, M], fitness_ref of each): computed once, read-only."""
    X, Y = span_table(M, n_var)
    exprs = [exact_exprs(p, n_var, SPAN_N_OUT) for p in range(SPAN_P)]
    want = np.stack([np.stack([value(e, X) for e in ex]) for ex in exprs])
    ref = np.array([fitness_ref(w, Y) for w in want])
    for a in (X, Y, want, ref):
        a.setflags(write=False)
    return X, Y, exprs, want, ref


@pytest.mark.parametrize("n_var", [8, 17])
@pytest.mark.parametrize("M", SPAN_M[1:])
def test_span_tables_tell_the_span_tree_from_a_left_fold(M, n_var):
    X, Y, _, want, ref = span_case(M, n_var)
    fold = np.array([fitness_ref(w, Y, left_fold=True) for w in want])
    assert np.all(np.isfinite(ref)) and np.all(ref < 1e4)  # nothing clipped: the bits are the sums'
    differ = int((ref.view(np.uint32) != fold.view(np.uint32)).sum())
    print(M, n_var, differ, "of", SPAN_P)
    assert 3 * differ >= SPAN_P, (differ, ref, fold)
