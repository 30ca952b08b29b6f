"""pybulletgym_amd: MI355X-native batched stepper for the roboschool locomotion envs of
josiahls/pybullet-gym (InvertedPendulum, InvertedPendulumSwingup, InvertedDoublePendulum,
Hopper, HalfCheetah, Ant, Humanoid, HumanoidFlagrun, HumanoidFlagrunHarder, Walker2D, Atlas
``*PyBulletEnv-v0``, and the MuJoCo-observation variants).  Import as ``import pybulletgym_amd``.

    from pybulletgym_amd import VecEnv, make
    envs = VecEnv("AntPyBulletEnv-v0", 16384)      # device-resident batch, one launch per step
    env = make("AntPyBulletEnv-v0")                  # single env, gym.Env-style surface
"""


def __getattr__(name):
    # lazy: keep `import pybulletgym_amd` cheap and torch-free for the model compiler
    if name == "ENV_IDS":  # the env ids in robot_id order (robots.py, the one robot registry)
        from . import robots
        return tuple(s.env_id for s in robots.BY_ID)
    if name == "VecEnv":
        from .vec_env import VecEnv
        return VecEnv
    if name == "MLPPolicy":
        from .policy import MLPPolicy
        return MLPPolicy
    if name == "MLPPopulation":
        from .policy import MLPPopulation
        return MLPPopulation
    if name == "EvolutionStrategy":
        from .es import EvolutionStrategy
        return EvolutionStrategy
    if name == "ActionNoise":
        from .policy import ActionNoise
        return ActionNoise
    if name == "PPO":
        from .ppo import PPO
        return PPO
    if name in ("make", "register_with_gym"):
        from . import envs
        return getattr(envs, name)
    raise AttributeError(name)
