"""tests/monitor_ref.py against cases worked by hand: the deque and its overflow inside one step, the target gating, the life-time totals, evaluate_policy's
bookkeeping and explained_variance.  No GPU, no library."""
import math

import numpy as np
import pytest

import monitor_ref as ref


def test_deque_in_environment_order_and_totals():
    m = ref.MonitorRef(4, window=3, horizon=10)
    assert m.step([0, 1, 0, 2], [9.0, 1.5, 9.0, -2.0], [7, 3, 7, 10]) == 2
    assert [tuple(map(float, r[:1])) + r[1:] for r in m.buffer] == [(1.5, 3, 1, 0), (-2.0, 10, 3, 0)]
    assert (m.episodes, m.length_sum, m.return_sum, m.truncated, m.launches) == (2, 13, -0.5, 1, 1)
    assert m.step([0, 0, 0, 0], [float("nan")] * 4, [0] * 4) == 0                # nothing done: stale words are not read
    assert (m.episodes, m.return_sum, m.launches) == (2, -0.5, 2)
    assert m.step([0xff, 0, 0x80, 0], [4.0, 1e30, 0.25, float("nan")], [12, 1, 2, 1]) == 2
    assert [r[1:] for r in m.buffer] == [(10, 3, 0), (12, 0, 2), (2, 2, 2)]       # window 3: the oldest of the four left
    s = m.summary()
    assert s["rollout/ep_rew_mean"] == (-2.0 + 4.0 + 0.25) / 3 and s["rollout/ep_len_mean"] == 8.0
    assert s["rollout/episodes"] == 4 and s["rollout/truncated"] == 2
    assert s["rollout/ep_rew_mean_all"] == 3.75 / 4 and s["rollout/ep_len_mean_all"] == 27 / 4
    rows = m.rows()
    assert rows.dtype == np.int32 and rows.shape == (3, 4) and rows[:, 0].view(np.float32).tolist() == [-2.0, 4.0, 0.25]


def test_window_overflows_inside_one_step():
    m = ref.MonitorRef(5, window=2)
    m.step([1] * 5, [0.0, 1.0, 2.0, 3.0, 4.0], [1] * 5)
    assert [(float(r[0]), r[2]) for r in m.buffer] == [(3.0, 3), (4.0, 4)] and m.episodes == 5 and m.return_sum == 10.0
    assert m.abs_sum_bound == 2.0 * 5 * 2.0 ** -53 * 10.0


def test_empty_monitor_means_are_nan():
    s = ref.MonitorRef(3, window=4).summary()
    assert all(math.isnan(s[k]) for k in ("rollout/ep_rew_mean", "rollout/ep_len_mean", "rollout/ep_rew_mean_all", "rollout/ep_len_mean_all"))
    assert s["rollout/episodes"] == 0


def test_target_gating():
    m = ref.MonitorRef(3, window=8, targets=[0, 1, 2])
    m.step([1, 1, 1], [1.0, 2.0, 3.0], [1, 1, 1])                                # environment 0 never counts
    m.step([1, 1, 1], [4.0, 5.0, 6.0], [1, 1, 1])                                # environment 1 has reached its target
    m.step([1, 1, 1], [7.0, 8.0, 9.0], [1, 1, 1])                                # so has environment 2
    assert [(float(r[0]), r[2], r[3]) for r in m.buffer] == [(2.0, 1, 0), (3.0, 2, 0), (6.0, 2, 1)]
    assert m.counts == [0, 1, 2] and m.episodes == 3 and m.launches == 3


@pytest.mark.parametrize("n_eval,n_envs", [(1, 64), (10, 4), (64, 64), (100, 64), (7, 3), (5, 1)])
def test_targets_sum_to_n(n_eval, n_envs):
    t = ref.eval_targets(n_eval, n_envs)
    assert len(t) == n_envs and sum(t) == n_eval and max(t) - min(t) <= 1 and t == sorted(t)


def test_sb3_bookkeeping_by_hand():
    # two environments, three episodes wanted: targets [1, 2]
    steps = [([0, 1], [0.0, 1.0], [0, 2]), ([1, 0], [2.0, 0.0], [3, 0]), ([1, 1], [3.0, 4.0], [1, 5]), ([1, 1], [5.0, 6.0], [1, 1])]
    rewards, lengths = ref.sb3_evaluate_bookkeeping(steps, 2, 3)
    assert rewards == [1.0, 2.0, 4.0] and lengths == [2, 3, 5]                   # environment 0's second episode (3.0) is past its target
    with pytest.raises(RuntimeError):
        ref.sb3_evaluate_bookkeeping(steps[:2], 2, 3)
    # the same through the monitor's gating
    m = ref.MonitorRef(2, window=3, targets=ref.eval_targets(3, 2))
    for d, r, l in steps:
        m.step(d, r, l)
    assert [float(x[0]) for x in m.buffer] == rewards and [x[1] for x in m.buffer] == lengths


def test_explained_variance():
    assert math.isnan(ref.explained_variance([1.0, 2.0, 3.0], [5.0, 5.0, 5.0]))  # zero variance of the returns
    assert math.isnan(ref.explained_variance([1.0], [2.0]))
    assert ref.explained_variance([1.0, 2.0, 4.0], [1.0, 2.0, 4.0]) == 1.0
    assert ref.explained_variance([0.0, 0.0], [1.0, 3.0]) == 0.0                 # a constant prediction explains nothing
    assert ref.explained_variance([3.0, 1.0], [1.0, 3.0]) == 1.0 - 4.0 / 1.0     # var(y - p) = 4, var(y) = 1
    y = np.float32(100.0) + np.arange(4, dtype=np.float32)
    assert ref.explained_variance(y + np.float32(0.5), y) == 1.0                 # a constant offset is explained
