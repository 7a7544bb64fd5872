"""The numpy path of UltrasoundVecEnv (step_async / step_wait: one packed block per step, include/usim.h usim_pack_step) against the tensor path of a second
environment with the same seed and the same actions: step_tensor plus direct reads of the tensor properties.  Both run the same step kernel on the same
inputs, so everything is compared for equality, not to a tolerance.

horizon 12 with early termination on: every environment finishes within the 40 steps, most steps have finished and running environments side by side, and
early termination ends episodes at irregular steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pair(usim, n, torso, seed=7, **opts):
    kw = dict(usim.default_robosuite_kwargs())
    env_kw = {k: opts.pop(k) for k in ("monitor", "report_truncation") if k in opts}
    kw.update(opts)
    host = usim.UltrasoundVecEnv(n, device=DEV, seed=seed, torso=torso, **env_kw, **kw)
    dev = usim.UltrasoundVecEnv(n, device=DEV, seed=seed, torso=torso, **kw)
    return host, dev


def _run(host, dev, steps, monitor=True, report_truncation=False):
    """drives both environments; returns the number of steps without / with finished environments"""
    n = host.num_envs
    g = np.random.default_rng(11)
    lo, hi = host.action_space.low, host.action_space.high
    o_h, o_d = host.reset(), dev.reset_tensor().cpu().numpy()
    assert o_h.tobytes() == o_d.tobytes()
    kept, quiet, busy = None, 0, 0
    for k in range(steps):
        a = (lo + (hi - lo) * g.random((n, host.action_dim))).astype(np.float32)
        before = host._d2h_transfers
        obs, rew, done, infos = host.step(a)
        transfers = host._d2h_transfers - before
        t_obs, t_rew, t_done = dev.step_tensor(torch.from_numpy(a).to(DEV))
        torch.cuda.synchronize()
        t_obs, t_rew, t_done = t_obs.cpu().numpy(), t_rew.cpu().numpy(), t_done.cpu().numpy()
        term, ep_r, ep_l = dev.terminal_obs.cpu().numpy(), dev.episode_return.cpu().numpy(), dev.episode_length.cpu().numpy()

        assert obs.dtype == np.float32 and obs.shape == (n, 19) and obs.flags["C_CONTIGUOUS"] and rew.dtype == np.float32 and rew.shape == (n,)
        assert done.dtype == np.bool_ and done.shape == (n,)
        assert obs.tobytes() == t_obs.tobytes() and rew.tobytes() == t_rew.tobytes() and np.array_equal(done, t_done != 0), f"step {k}"
        assert isinstance(infos, list) and len(infos) == n and len({id(d) for d in infos}) == n
        keys = {"terminal_observation"} | ({"episode"} if monitor else set()) | ({"TimeLimit.truncated"} if report_truncation else set())
        for i in range(n):
            if not done[i]:
                assert infos[i] == {}, (k, i)
                continue
            assert set(infos[i]) == keys, (k, i)
            t = infos[i]["terminal_observation"]
            assert t.dtype == np.float32 and t.tobytes() == term[i].tobytes(), (k, i)
            if monitor:
                ep = infos[i]["episode"]
                assert set(ep) == {"r", "l", "t"} and type(ep["r"]) is float and type(ep["l"]) is int and ep["t"] >= 0.0
                assert ep["r"] == float(ep_r[i]) and ep["l"] == int(ep_l[i]), (k, i)
            if report_truncation:
                assert infos[i]["TimeLimit.truncated"] is bool(ep_l[i] >= host.horizon), (k, i)
        assert transfers == (2 if done.any() else 1), (k, transfers, int(done.sum()))
        quiet, busy = quiet + (not done.any()), busy + bool(done.any())

        if kept is not None:                                      # what step k - 1 returned is untouched by step k: nothing aliases the pinned mirror
            for arr, snap in kept:
                assert arr.tobytes() == snap
        kept = [(x, x.tobytes()) for x in (obs, rew, done)] + [(d["terminal_observation"], d["terminal_observation"].tobytes()) for d in infos if d]
    return quiet, busy


@pytest.mark.parametrize("opts", [{}, {"report_truncation": True}, {"monitor": False}, {"monitor": False, "report_truncation": True}],
                         ids=["default", "report_truncation", "no_monitor", "no_monitor_report_truncation"])
def test_numpy_path_equals_tensor_path_soft_torso(usim, opts):
    n = 67
    host, dev = _pair(usim, n, "soft", horizon=12, **opts)
    try:
        quiet, busy = _run(host, dev, 40, monitor=opts.get("monitor", True), report_truncation=opts.get("report_truncation", False))
        assert busy >= 3                                          # the horizon alone ends every episode three times in 40 steps
    finally:
        host.close(); dev.close()


@pytest.mark.parametrize("torso", ["rigid", "full"])
def test_numpy_path_equals_tensor_path_other_torsos(usim, torso):
    host, dev = _pair(usim, 8, torso, horizon=4, early_termination=False)
    try:
        quiet, busy = _run(host, dev, 6)
        assert (quiet, busy) == (5, 1)                            # every episode ends at step 4
    finally:
        host.close(); dev.close()


def test_one_transfer_per_step_two_where_an_episode_ended(usim):
    """horizon 12 without early termination: steps 1 - 11 end no episode, step 12 ends all of them"""
    kw = dict(usim.default_robosuite_kwargs(), horizon=12, early_termination=False)
    env = usim.UltrasoundVecEnv(67, device=DEV, seed=7, torso="soft", **kw)
    try:
        env.reset()
        a = np.full((67, env.action_dim), 0.5, dtype=np.float32)
        assert env._d2h_transfers == 0
        for k in range(1, 25):
            before = env._d2h_transfers
            env.step_async(a)
            _, _, done, infos = env.step_wait()
            assert done.all() == (k % 12 == 0) and done.any() == done.all()
            assert env._d2h_transfers - before == (2 if k % 12 == 0 else 1), k
            assert all(bool(d) == (k % 12 == 0) for d in infos)
        with pytest.raises(RuntimeError):
            env.step_wait()
    finally:
        env.close()
