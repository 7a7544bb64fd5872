"""ppo.NativePPO's continual training end to end (src/rl.py:148-167) on 64 environments x 8 steps, minibatch 128, two epochs: a checkpoint written by one
learner and restored IN PLACE by another gives the same next update bit for bit; target_kl stops an update from the device with update() still returning
exactly STAT_NAMES; learn() after set_checkpointing(...) writes CheckpointCallback's files."""
import io
import zipfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N, T, BATCH, EPOCHS = 64, 8, 128, 2
BUFFER = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")
VN = ("obs_mean", "obs_var", "_obs_count", "ret_mean", "ret_var", "_ret_count")


def _setup(usim, seed=0, **kw):
    pol, ppo = usim.policy, usim.ppo
    env = usim.UltrasoundVecEnv(N, device="cuda:0", seed=3, torso="rigid", **usim.default_robosuite_kwargs())
    dev = env.device
    torch.manual_seed(seed)
    policy = pol.MlpActorCritic(19, env.action_dim).to(dev)
    for m in policy.modules():                                             # SB3's initialisation, as tools/ppo_demo.py
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.orthogonal_(m.weight, gain=2 ** 0.5); torch.nn.init.zeros_(m.bias)
    torch.nn.init.orthogonal_(policy.action_net.weight, gain=0.01); torch.nn.init.orthogonal_(policy.value_net.weight, gain=1.0)
    ppo.flatten_parameters(policy)
    vn = pol.DeviceVecNormalize(N, 19, device=dev, training=True, norm_reward=True)
    buf = pol.DeviceRolloutBuffer(T, N, 19, env.action_dim, device=dev)
    coll = pol.FusedRollout(env, policy, vn, buf, seed=seed)
    kw = dict(dict(n_epochs=EPOCHS, batch_size=BATCH), **kw)
    return env, ppo.NativePPO(env, policy, vn, buf, coll, seed=seed, **kw)


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def test_a_restored_learner_makes_the_same_update(usim, tmp_path):
    """A: learn(2), save_checkpoint, collect(), update().  B (another initialisation, fresh statistics): load_checkpoint, A's buffer and generator state,
    update().  theta, both moments and the step count are then bit-equal.  The VecNormalize tensors are compared with A's AT THE CHECKPOINT: A's collect() after
    it moves A's statistics on, and update() touches neither's."""
    env_a, a = _setup(usim, seed=0)
    a.learn(2)
    zip_path, pkl_path = a.save_checkpoint(tmp_path, "tracking")
    assert zip_path.name == "tracking.zip" and pkl_path.name == "vec_normalize_tracking.pkl"
    vn_saved = {k: getattr(a.vecnorm, k).clone() for k in VN}
    a.collector.collect()
    buffer = {k: getattr(a.buffer, k).clone() for k in BUFFER}
    gen = a.generator.get_state()
    out_a = a.update()
    torch.cuda.synchronize()

    env_b, b = _setup(usim, seed=5)
    assert not torch.equal(a.theta, b.theta)
    ptrs = [p.data_ptr() for p in b.policy.parameters()] + [b.theta.data_ptr(), b.exp_avg.data_ptr(), b.step_count.data_ptr()] + \
           [getattr(b.vecnorm, k).data_ptr() for k in VN]
    b.vecnorm.returns.fill_(1.5)
    data = b.load_checkpoint(tmp_path, "tracking", reset_num_timesteps=False)
    assert b.num_timesteps == 2 * N * T == data["num_timesteps"] and data["n_epochs"] == EPOCHS and data["batch_size"] == BATCH
    for k in VN:
        assert torch.equal(_bits(getattr(b.vecnorm, k)), _bits(vn_saved[k])), k
    assert not b.vecnorm.returns.any()
    assert ptrs == [p.data_ptr() for p in b.policy.parameters()] + [b.theta.data_ptr(), b.exp_avg.data_ptr(), b.step_count.data_ptr()] + \
           [getattr(b.vecnorm, k).data_ptr() for k in VN]                   # the same views: what the collector recorded is still where the weights are
    assert usim.ppo._is_flat(b.policy, b.theta)
    for k in BUFFER:
        getattr(b.buffer, k).copy_(buffer[k])
    b.buffer.full = True
    b.generator.set_state(gen)
    out_b = b.update()
    torch.cuda.synchronize()
    assert out_a == out_b and tuple(out_b) == usim.ppo.STAT_NAMES
    for k in ("theta", "exp_avg", "exp_avg_sq", "step_count"):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k
    assert int(b.step_count.item()) == 3 * EPOCHS * (N * T // BATCH)
    assert a.last_update == b.last_update and b.last_update["train/optimizer_steps"] == b.last_update["train/minibatches_evaluated"] == EPOCHS * (N * T // BATCH)
    assert b.last_update["train/early_stop"] == 0 and b.last_update["train/clip_range"] == 0.2 and "train/clip_range_vf" not in b.last_update
    assert b.last_update["train/std"] == pytest.approx(float(torch.exp(b.policy.log_std.detach()).mean()), rel=1e-6)
    assert {"train/std", "train/optimizer_steps", "train/early_stop"} <= set(a.history[-1])
    b.collector.collect()                                                  # the collector recorded before the load goes on working, on the restored weights
    with torch.no_grad():
        _, value = b.policy.forward(b.buffer.observations[0])
    assert torch.allclose(b.buffer.values[0], value, atol=3e-5)
    # the zip is a stable-baselines3 checkpoint: load_sb3_zip, and the optimizer state under torch.load(weights_only=True)
    sd, _ = usim.policy.load_sb3_zip(zip_path)
    assert list(sd) == list(a.policy.to_sb3_state_dict())
    with zipfile.ZipFile(zip_path) as z:
        opt = torch.load(io.BytesIO(z.read("policy.optimizer.pth")), map_location="cpu", weights_only=True)
    assert len(opt["state"]) == 13 and opt["state"][0]["step"] == 2 * EPOCHS * (N * T // BATCH)
    st = usim.policy.load_vecnormalize_pkl(pkl_path)
    assert np.array_equal(st["obs_mean"], vn_saved["obs_mean"].cpu().numpy()) and st["count"] == float(vn_saved["_obs_count"])
    env_a.close(); env_b.close()


def test_target_kl_stops_the_update_on_the_device(usim):
    """Two learners of one seed collect the same buffer.  Its log_probs are lowered by 0.25 in both, as if the policy had moved since the rollout (approx_kl =
    e^0.25 - 1 - 0.25 = 0.034).  The first measures the first minibatch's approx_kl; the second runs with target_kl at a third of it (1.5 target_kl = half)."""
    kl = None
    for target in (None, "measured"):
        env, ln = _setup(usim, seed=1, **({} if target is None else dict(target_kl=kl / 3.0)))
        ln.collector.collect()
        ln.buffer.log_probs.sub_(0.25)
        theta0, m0 = ln.theta.clone(), ln.exp_avg.clone()
        out = ln.update()
        torch.cuda.synchronize()
        assert tuple(out) == usim.ppo.STAT_NAMES
        if target is None:
            kl = float(ln.first_stats[3])
            assert 0.02 < kl < 0.05 and ln.last_update["train/early_stop"] == 0 and not torch.equal(ln.theta, theta0)
            assert ln.last_update["train/optimizer_steps"] == EPOCHS * (N * T // BATCH)
        else:
            lu = ln.last_update
            assert lu["train/early_stop"] == 1 and lu["train/optimizer_steps"] == 0 and lu["train/minibatches_evaluated"] == 1
            assert torch.equal(_bits(ln.theta), _bits(theta0)) and torch.equal(_bits(ln.exp_avg), _bits(m0)) and int(ln.step_count.item()) == 0
            assert out["train/approx_kl"] == kl                            # the statistics of the tripping minibatch -- the same first minibatch, the same bits
            assert torch.equal(_bits(ln.stats), _bits(ln.first_stats))
        env.close()


def test_learn_writes_checkpoint_callback_files(usim, tmp_path):
    env, ln = _setup(usim, seed=2)
    rollout = N * T
    ln.set_checkpointing(rollout, checkpoint_dir=tmp_path / "ck", name_prefix="rl_model")
    ln.learn(3)
    names = sorted(p.name for p in (tmp_path / "ck").iterdir())
    steps = [rollout, 2 * rollout, 3 * rollout]
    assert names == sorted([f"rl_model_{s}_steps.zip" for s in steps] + [f"vec_normalize_rl_model_{s}_steps.pkl" for s in steps])
    assert usim.policy.load_sb3_zip(tmp_path / "ck" / f"rl_model_{steps[1]}_steps.zip")[1]["num_timesteps"] == steps[1]
    env2, other = _setup(usim, seed=2)
    other.set_checkpointing(2 * rollout, checkpoint_dir=tmp_path / "ck2")
    other.learn(3)                                                         # every further multiple reached or passed: after iterations 2 only
    assert sorted(p.name for p in (tmp_path / "ck2").iterdir()) == [f"rl_model_{steps[1]}_steps.zip", f"vec_normalize_rl_model_{steps[1]}_steps.pkl"]
    assert torch.equal(_bits(ln.theta), _bits(other.theta))                # saving changes nothing
    env.close(); env2.close()
