"""The broad phase of the collision (csrc/usim_kernels.hip collide_cull) only filters what the exact narrow phase then decides: an element it drops cannot touch
the probe, so the contact lists are those of walking all 99 elements.  Checked where there is most contact: 64 environments over the first 60 steps after a
synchronous reset (every probe spawns in touch; this is where the eight contact slots overflow).

Every step, the contact count and shell ids of the split kernel (16-lane groups) equal
  - the float64 oracle's, which has no broad phase, under the rule of tests/test_gpu_parity.py: a difference must be explained by the oracle's own margin to a
    threshold (razor edge), is counted, must be rare, and excludes the environment from then on;
  - those of the 8-lane split kernel and of the single-wave 16-lane kernel, bit for bit on every environment, together with the done flags and observations."""
import numpy as np
import pytest

from test_gpu_parity import _mk, _razor_edge

pytestmark = pytest.mark.gpu

N, STEPS = 64, 60
CASES = {"shipped": {},
         "randomised": dict(friction_randomization=1),                            # friction drawn per episode, on top of the shipped stiffness / damping draws
         "wide_blade": dict(probe_halfwidth=0.01, probe_tip=0.005)}                # the general form of the cull constant: sideways sweep, tip beyond the site


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", list(CASES))
def test_contact_lists_are_the_exact_ones(usim, case):
    extra = CASES[case]
    env, ora = _mk(usim, N, "soft", "tracking", **extra)
    others = {lanes: _mk(usim, N, "soft", "tracking", gpu_extra=dict(lanes_per_env=lanes), **extra)[0] for lanes in (64, 16)}
    env.reset(); ora.reset()
    for o in others.values():
        o.reset()
    alive = np.ones(N, dtype=bool)
    explained = contacts = full = 0
    for k in range(STEPS):
        a = ora.random_actions(k)
        _, _, done_o, _, con_o = ora.step(a)
        obs_g, _, done_g, _ = env.step(a.astype(np.float32))
        con_g = env.contacts.cpu().numpy()
        for lanes, o in others.items():
            obs_x, _, done_x, _ = o.step(a.astype(np.float32))
            assert np.array_equal(o.contacts.cpu().numpy(), con_g), f"step {k}: contact lists of lanes_per_env {lanes} differ from the split kernel's"
            assert np.array_equal(done_x, done_g) and np.array_equal(_bits(obs_x), _bits(obs_g)), f"step {k}: lanes_per_env {lanes}"
        mism = ((done_g != done_o) | (con_g != con_o).any(1)) & alive
        if mism.any():
            inf = ora.last_info()
            for i in np.nonzero(mism)[0]:
                assert _razor_edge(inf, i), f"env {i} step {k}: contacts {con_g[i]} / oracle {con_o[i]}, contact margin {inf['contact_margin'][i]}"
                explained += 1
            alive &= ~mism
        assert np.array_equal(con_g[alive], con_o[alive]) and np.array_equal(done_g[alive], done_o[alive])
        contacts += int(con_o[:, 0].sum()); full += int((con_o[:, 0] == 8).sum())
    print(f"{case}: {contacts} contacts over {N} x {STEPS} env-steps, {full} env-steps with all eight slots taken, {explained} razor edges")
    assert contacts > 0                                                             # the lists are not trivially empty
    assert explained <= max(1, N // 50)                                             # rare (the parity tests' share: 1 % of the environments, at least one)
    env.close()
    for o in others.values():
        o.close()
