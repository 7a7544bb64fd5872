"""MI355X-native batched simulator of the reference's `Ultrasound` environment (hot path only).

    env = UltrasoundVecEnv(4096, device="cuda:0", seed=3, **robosuite_block_of_rl_config_yaml)
    obs = env.reset(); obs, rew, done, infos = env.step(actions)        # stable-baselines3 VecEnv protocol
    obs_t, rew_t, done_t = env.step_tensor(actions_t)                    # torch tensors, no host sync

The compute path is libusim.so (HIP kernels for gfx950 behind the C ABI of include/usim.h); importing this
package without it raises."""
from . import _lib
from .config import default_robosuite_kwargs, load_yaml, make_config
from .spaces import Box
from .vec_env import UltrasoundEnv, UltrasoundVecEnv

from . import episode_log, error_metrics, evaluation, imitation, learner, monitor, planner, policy, ppo  # noqa: E402  (checkpoint readers, on-device VecNormalize, MLP policy replay, MPPI planner, the learners' flat block and core, PPO learner, behaviour cloning + DAgger, episode statistics + evaluation, CSV dump, error metrics, their device-side evaluation runs)
from .monitor import DeviceMonitor, evaluate_policy, write_scalar_csv  # noqa: E402
from .evaluation import DeviceEpisodeMetrics, EpisodeRecorder, evaluate_episodes  # noqa: E402
from .imitation import DAggerTrainer, DemoBuffer, NativeBC, PlannerExpert, PolicyExpert, distill  # noqa: E402
from . import population  # noqa: E402  (K policies in one rollout: evaluated and trained side by side)
from .population import PolicyPopulation, PopulationPPO, PopulationRollout, PopulationVecNormalize, evaluate_population  # noqa: E402

__all__ = ["UltrasoundVecEnv", "UltrasoundEnv", "Box", "default_robosuite_kwargs", "load_yaml", "make_config", "policy", "planner", "ppo", "monitor", "DeviceMonitor",
           "evaluate_policy", "write_scalar_csv", "episode_log", "error_metrics", "evaluation", "DeviceEpisodeMetrics", "EpisodeRecorder", "evaluate_episodes", "imitation", "learner", "DemoBuffer", "NativeBC",
           "PolicyExpert", "PlannerExpert", "DAggerTrainer", "distill", "population", "PolicyPopulation", "PopulationVecNormalize",
           "PopulationRollout", "PopulationPPO", "evaluate_population", "_lib"]
