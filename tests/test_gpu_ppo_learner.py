"""ppo.NativePPO end to end on a small problem: rigid torso, 64 environments x 32 steps, policy.FusedRollout as the collector.  The kernels' arithmetic is
test_gpu_ppo_kernels.py's subject; here: the flat block, the module and the collector stay one memory through an update, an update learns, the trailing partial
minibatch is consumed, a checkpoint carries the weights and Adam's moments bit for bit, and a seed fixes the result."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N, T = 64, 32


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
    theta = ppo.flatten_parameters(policy)
    vn = pol.DeviceVecNormalize(N, 19, device=dev, training=True, norm_reward=True)
    buf = pol.DeviceRolloutBuffer(T, N, 19, env.action_dim, device=dev)
    coll = pol.FusedRollout(env, policy, vn, buf, seed=seed)
    learner = ppo.NativePPO(env, policy, vn, buf, coll, seed=seed, **kw)
    assert learner.theta is theta
    return env, policy, coll, learner


@pytest.fixture(scope="module")
def trained(usim):
    """one collect() and one update() of ten epochs on that buffer, with what the tests below look at"""
    env, policy, coll, learner = _setup(usim)
    coll.collect()
    theta0, packed0 = learner.theta.clone(), coll._w2_packed.clone()
    out = learner.update()
    torch.cuda.synchronize()
    yield dict(env=env, policy=policy, coll=coll, learner=learner, theta0=theta0, packed0=packed0, out=out)
    env.close()


def test_update_returns_sb3_names(usim, trained):
    out = trained["out"]
    assert tuple(out) == usim.ppo.STAT_NAMES and all(np.isfinite(v) for v in out.values())
    assert out["train/value_loss"] > 0 and out["train/entropy_loss"] < 0 and 0 <= out["train/clip_fraction"] <= 1
    assert int(trained["learner"].step_count.item()) == 10 * 8             # batch_size None: eight minibatches per epoch


def test_module_theta_and_collector_agree_after_an_update(usim, trained):
    learner, policy, coll = trained["learner"], trained["policy"], trained["coll"]
    theta = learner.theta
    assert not torch.equal(theta, trained["theta0"])                        # the update moved the parameters ...
    assert usim.ppo._is_flat(policy, theta)                                 # ... and the module's parameters are still the views
    o = 0
    for _, path in usim.ppo.FIELDS:
        p = dict(policy.named_parameters())[path]
        assert torch.equal(p.detach().reshape(-1), theta[o:o + p.numel()])
        o += p.numel()
    assert not torch.equal(coll._w2_packed, trained["packed0"])             # pack() ran after the last step: the collector's operands are the new weights'
    coll.collect()
    b = coll.buffer
    with torch.no_grad():
        _, value = policy.forward(b.observations[0])
        stale = usim.policy.MlpActorCritic(19, trained["env"].action_dim).to(theta.device)
        usim.ppo.flatten_parameters(stale).copy_(trained["theta0"])
        _, old_value = stale.forward(b.observations[0])
    assert torch.allclose(b.values[0], value, atol=3e-5), float((b.values[0] - value).abs().max())          # what the collector computed is the module's value
    assert float((b.values[0] - old_value).abs().max()) > 1e-3              # (and not that of the parameters before the update)


def test_ten_epochs_lower_the_value_loss(usim):
    """Ten epochs on one fixed buffer, the whole buffer as the minibatch: the first and the last minibatch are then the SAME 2048 samples and their value losses
    differ by what the ten steps learnt.  (Between two different minibatches of 256 the loss differs by sampling noise -- about a tenth of it -- which is more than
    eighty steps at learning rate 3e-4 move it: a comparison across them would test the shuffle.)"""
    env, policy, coll, learner = _setup(usim, batch_size=N * T)
    coll.collect()
    out = learner.update()
    first, last = float(learner.first_stats[1]), out["train/value_loss"]
    print(f"value loss: first minibatch {first:.6f}, last {last:.6f}")
    assert int(learner.step_count.item()) == 10 and last < first, (first, last)
    env.close()


def test_save_returns_weights_and_moments_bit_for_bit(usim, trained, tmp_path):
    learner, policy = trained["learner"], trained["policy"]
    path = tmp_path / "model.zip"
    learner.save(path)
    sd, _ = usim.policy.load_sb3_zip(path)
    want = policy.to_sb3_state_dict()
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in sd)
    import io, zipfile
    with zipfile.ZipFile(path) as z:
        opt = torch.load(io.BytesIO(z.read("policy.optimizer.pth")), map_location="cpu", weights_only=True)
    names, offsets, o = list(policy.state_dict()), {}, 0
    params = dict(policy.named_parameters())
    for _, p in usim.ppo.FIELDS:
        offsets[p] = o
        o += params[p].numel()
    assert len(opt["state"]) == 13 and opt["param_groups"][0]["params"] == list(range(13)) and opt["param_groups"][0]["eps"] == 1e-5
    for i, name in enumerate(names):
        st, n = opt["state"][i], params[name].numel()
        assert st["step"] == 80 and st["exp_avg"].shape == params[name].shape
        assert torch.equal(st["exp_avg"].reshape(-1), learner.exp_avg[offsets[name]:offsets[name] + n].cpu())
        assert torch.equal(st["exp_avg_sq"].reshape(-1), learner.exp_avg_sq[offsets[name]:offsets[name] + n].cpu())
    assert float(learner.exp_avg.abs().max()) > 0


def test_a_trailing_partial_minibatch_is_consumed(usim):
    env, policy, coll, learner = _setup(usim, n_epochs=1, batch_size=600)    # 2048 = 600 + 600 + 600 + 248
    coll.collect()
    calls = []
    step = learner.minibatch_step
    learner.minibatch_step = lambda data, index, batch, lr=None: (calls.append((int(batch), int(index.numel()))), step(data, index, batch, lr))[1]
    learner.update()
    assert calls == [(600, 600)] * 3 + [(248, 248)] and int(learner.step_count.item()) == 4
    env.close()


def test_the_same_seed_gives_the_same_parameters(usim):
    thetas = []
    for _ in range(2):
        env, policy, coll, learner = _setup(usim, seed=7, n_epochs=2)
        learner.learn(2)
        torch.cuda.synchronize()
        thetas.append(learner.theta.clone())
        env.close()
    assert torch.equal(thetas[0].view(torch.int32), thetas[1].view(torch.int32)) and torch.isfinite(thetas[0]).all()
