"""PointwiseEvaluator(wide=True): the opt-in flag, the widened limits of prepare and of the C entries (refusals
before any device call), and the unchanged ABI version."""
import ctypes

import numpy as np
import pytest

import multitreegp_amd as mt
from multitreegp_amd import _native as nat


def table(n_var):
    return np.zeros((5, n_var), np.float32), np.zeros((5, 1), np.float32)


def test_wide_is_opt_in_and_prepares_up_to_64_columns():
    assert mt.PointwiseEvaluator().wide is False
    with pytest.raises(NotImplementedError):
        mt.PointwiseEvaluator().prepare(table(9))
    ff = mt.PointwiseEvaluator(wide=True)
    d = ff.prepare(table(64))
    assert d["xt"].shape == (64, d["ld"]) and (d["n_var"], ff.n_data(), nat.PW_WIDE_MAX_VAR) == (64, 64, 64)
    with pytest.raises(NotImplementedError):
        ff.prepare(table(65))


@pytest.mark.parametrize("n_var, chain_next, want", [(65, 0, nat.ERR_ARG), (9, 1, nat.ERR_ARG)])
def test_c_entries_refuse_before_any_device_call(n_var, chain_next, want):
    assert nat.ABI_VERSION == 24
    lib = nat.load()
    buf = np.zeros(64, np.float32)  # host memory, 16-byte aligned view: a launch would fault, a refusal reads nothing
    ptr = (buf.ctypes.data + 15) // 16 * 16
    pw = nat.MtgpPointwise()
    pw.xt = pw.yt = pw.nodes = pw.fitness = ptr
    pw.M, pw.ld, pw.n_var, pw.n_out, pw.max_fitness = 4, 4, n_var, 2, 1.0
    jc = nat.MtgpJitCode()
    jc.code = jc.offsets = ptr
    jc.chain.next = chain_next
    sc = nat.MtgpPointwiseScale()
    args = (ptr, ptr, 2, 4, 1)
    if not chain_next:  # (the entries without code have no chain to refuse)
        assert lib.mtgp_eval_pointwise(ctypes.byref(pw), *args, None) == want
        assert lib.mtgp_eval_pointwise_scaled(ctypes.byref(pw), ctypes.byref(sc), *args, None) == want
    assert lib.mtgp_eval_pointwise_jit(ctypes.byref(pw), *args, ctypes.byref(jc), None) == want
    assert lib.mtgp_eval_pointwise_scaled_jit(ctypes.byref(pw), ctypes.byref(sc), *args, ctypes.byref(jc), None) == want
