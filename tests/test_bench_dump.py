"""bench.py --dump-outputs: float32 .npy files of what a timed step returned -- fitness and the
Dopri5 step counts whole, the trajectories on one seeded sample of lanes shared by every tensor,
within the byte budget, the same elements from run to run, and every file finite: <name>.npy with
0 at the non-finite elements plus <name>_nonfinite.npy with their class restore the array exactly."""
import os

import numpy as np
import torch

import bench

NAMES = ("fitness", "steps", "xs", "ys", "us", "acts")


def _result(P, R, S, lane_major, seed=0):
    g = torch.Generator().manual_seed(seed)
    res = {"fitness": torch.rand((P,), generator=g), "steps": torch.randint(0, 1000, (P, R), generator=g).int()}
    for name, c in (("xs", 4), ("ys", 4), ("us", 1), ("acts", 2)):
        t = torch.rand((S, c, P * R), generator=g) - 0.5
        t[S // 2:, :, 1::5] = float("inf")  # blown-up lanes: +-inf / NaN from some save point on
        t[S // 2:, 0, 2::5] = float("-inf")
        t[S - 1, :, 3::5] = float("nan")
        # lane-major: the adaptive solves' storage, a permuted view of a [P*R, S, c] buffer
        res[name] = t.permute(2, 0, 1).contiguous().permute(1, 2, 0) if lane_major else t
    res["fitness"][0] = float("inf")
    return res


def _load(d, k):
    """the dumped array put back together from its two finite files"""
    vals, kind = np.load(d / f"{k}.npy"), np.load(d / f"{k}_nonfinite.npy")
    for a in (vals, kind):
        assert a.dtype == np.float32 and a.flags.c_contiguous and np.isfinite(a).all(), k
    assert vals.shape == kind.shape and np.isin(kind, (0, 1, -1, 2)).all() and not vals[kind != 0].any(), k
    out = vals.copy()
    out[kind == 1], out[kind == -1], out[kind == 2] = np.inf, -np.inf, np.nan
    return out


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


def test_small_outputs_are_dumped_whole(tmp_path):
    P, R, S = 5, 3, 7
    for lane_major in (False, True):
        res = _result(P, R, S, lane_major)
        out = tmp_path / f"d{int(lane_major)}"
        bench.dump_outputs(str(out), res, res["fitness"], P, R)
        assert sorted(os.listdir(out)) == sorted(f"{k}{s}.npy" for k in NAMES for s in ("", "_nonfinite"))
        for k in NAMES:
            want = res[k].contiguous().numpy().astype(np.float32)
            assert _same(_load(out, k), want), k
        assert not np.isfinite(_load(out, "xs")).all() and np.isinf(_load(out, "fitness")[0])


def test_large_trajectories_keep_one_seeded_lane_sample(tmp_path, monkeypatch):
    P, R, S = 16, 8, 5
    lane_bytes = S * (4 + 4 + 1 + 2) * 4
    monkeypatch.setattr(bench, "DUMP_TRAJ_BYTES", 10 * lane_bytes + 3)  # room for 10 of the 128 lanes
    res = _result(P, R, S, False)
    bench.dump_outputs(str(tmp_path / "a"), res, res["fitness"], P, R)
    bench.dump_outputs(str(tmp_path / "b"), _result(P, R, S, True), res["fitness"], P, R)
    lanes = np.sort(np.random.default_rng(0).choice(P * R, 10, replace=False))
    total = 0
    for k in ("xs", "ys", "us", "acts"):
        a, b = _load(tmp_path / "a", k), _load(tmp_path / "b", k)
        total += a.nbytes
        assert a.shape == (S, res[k].shape[1], 10)
        assert _same(a, res[k].numpy()[:, :, lanes]), k
        assert _same(a, b), k  # either storage, same elements
    assert total <= 10 * lane_bytes + 3
    assert _load(tmp_path / "a", "fitness").shape == (P,)


def test_dump_budget_is_under_64_mb_with_the_whole_fitness_and_step_counts():
    # C3 at 8 ranks: 65,536 gathered fitness values + the rank's 8,192 x 32 step counts; each array
    # is written as two files of its size
    assert 2 * (bench.DUMP_TRAJ_BYTES + 65536 * 4 + 8192 * 32 * 4) <= 64 * 10 ** 6
