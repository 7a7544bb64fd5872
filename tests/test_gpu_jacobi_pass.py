"""The Jacobi pass of the top-face contact solve computes the same bits in every mapping (the promise of the comment over delassus_product in csrc/usim_contact.h):
the split kernel of 16-lane groups (lanes_per_env 32: one contact per lane, the summed directions in the quad layout, the tangent rows as a pair), the single-wave
16-lane kernel (lanes_per_env 16: one contact per lane, two row broadcasts per word, scalar tangent rows) and 8-lane groups (lanes_per_env 64: both contacts of a pair
in one lane).  64 environments, seed 3, 200 steps from reset, cold and with a warm start at 18 iterations.

The probe is pressed in right after the reset, so the run is meant to hold both wave-level cases of the solve, and the test asserts that it does: a wave (four
consecutive environments) in which some environment has at least five contacts -- the product summed by halves -- and a wave in contact whose four environments all
have at most four.  The mapping tests of test_gpu_warm_start.py and test_gpu_properties.py already hold all three pairs of mappings to the same bits, so all three
pairs are asserted here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, STEPS, SEED = 64, 200, 3
MAPPINGS = (32, 64, 16)


def _rollout(usim, lanes, extra):
    opts = dict(usim.default_robosuite_kwargs())
    opts.update(extra)
    env = usim.UltrasoundVecEnv(N, device="cuda:0", seed=SEED, torso="soft", lanes_per_env=lanes, **opts)
    env.reset_tensor()
    out = []
    for k in range(STEPS):
        obs, rew, done = env.step_tensor(env.random_actions_tensor(k))
        out.append((obs.clone(), rew.clone(), done.clone(), env.contacts.clone()))
    torch.cuda.synchronize()
    env.close()
    return [torch.stack(x) for x in zip(*out)]


@pytest.mark.parametrize("extra", [dict(), dict(warm_start=1, pgs_iters=18)], ids=["cold", "warm18"])
def test_mappings_agree_bit_for_bit_through_both_wave_level_cases(usim, extra):
    runs = {lanes: _rollout(usim, lanes, extra) for lanes in MAPPINGS}
    count = runs[32][3][:, :, 0].reshape(STEPS, N // 4, 4)               # contacts per environment, by step and wave of the 16-lane mappings
    most = count.max(dim=2).values
    print("largest contact count", int(count.max()), "; waves by largest count", torch.bincount(most.flatten().long(), minlength=9).tolist())
    assert (most >= 5).any(), "no wave with an environment of five or more contacts"
    assert ((most >= 1) & (most <= 4)).any(), "no wave in contact whose environments all have at most four"
    for a, b in ((32, 64), (32, 16), (64, 16)):
        for name, x, y in zip(("obs", "reward", "done", "contacts"), runs[a], runs[b]):
            diff = int((x != y).sum()) if x.dtype != torch.float32 else int((x.view(torch.int32) != y.view(torch.int32)).sum())
            print(f"lanes_per_env {a} vs {b}: {name} differs in {diff} words")
            assert diff == 0, (a, b, name)
