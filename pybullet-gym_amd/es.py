"""Evolution-strategy training on the device (Salimans et al. 2017, "Evolution Strategies as a Scalable
Alternative to Reinforcement Learning", mirrored sampling and centred ranks).

A generation perturbs the centre ``theta`` into ``n_pairs`` mirrored pairs ``theta +- sigma eps_i``
(``MLPPopulation.perturb``), runs every member for ``steps`` closed-loop env steps on its own group of
envs (``VecEnv.rollout``), turns the per-member mean returns into centred ranks and moves the centre by
``lr / (n_pairs sigma) * sum_i (rank[2 i] - rank[2 i + 1]) eps_i`` (``MLPPopulation.grad`` regenerates
the noise, nothing is stored).  Everything runs on the env's stream without a host synchronisation; the
run is a function of ``seed`` (and ``init_q``) alone and repeats bit for bit."""
from __future__ import annotations

import torch

from . import _native


class EvolutionStrategy:
    """``env``: a ``VecEnv`` whose ``num_envs`` is a multiple of ``population.n_members`` (with
    ``autoreset=False`` a member's fitness is its envs' mean first-episode return, with ``autoreset=True``
    the mean return over the ``steps`` window).  ``population``: an ``MLPPopulation`` on the env's device
    mapping the env's observation to its action.  ``sigma``: the perturbations' standard deviation;
    ``lr``: the step size; ``steps``: env steps per rollout; ``seed``: of the initial centre
    (``population.init_theta``) and of the noise.  ``init_q``: ``[num_envs, reset_dofs]`` joint positions
    every reset starts from (None: the env's own reset noise, fresh each generation).
    ``obs_norm=True``: running observation normalisation (Salimans et al. 2017, Mania et al. 2018): an
    ``ObsStats`` (``obs_stats``) is attached to the population during ``step()``'s rollouts, and after each
    generation's rollout it is finalized into the population's normaliser (``clip`` = ``obs_clip``), so
    generation g + 1 acts under the statistics of generations 0 .. g, all members under the same ones;
    generation 0 under the initial totals (mean 0, inv_std 1).  ``evaluate()`` does not move the statistics.

    ``theta`` (device float32 ``[n_params]``) is the centre and ``generation`` the number of ``step()``
    calls so far; both may be assigned (to resume a run)."""

    def __init__(self, env, population, sigma: float, lr: float, steps: int, seed: int = 0, init_q=None,
                 obs_norm: bool = False, obs_clip: float = 5.0):
        env_idx = env.device.index if env.device.index is not None else torch.cuda.current_device()
        if population.device != torch.device("cuda", env_idx):
            raise _native.PbgError(f"EvolutionStrategy: the population is on {population.device}, the env on {env.device}")
        if env.num_envs % population.n_members != 0:
            raise _native.PbgError(f"EvolutionStrategy: {env.num_envs} envs are not a multiple of the population's "
                                   f"{population.n_members} members")
        if (population.obs_dim, population.act_dim) != (env.info.obs_dim, env.info.action_dim):
            raise _native.PbgError(f"EvolutionStrategy: the population maps {population.obs_dim} -> {population.act_dim}, "
                                   f"the env's obs_dim / action_dim are {env.info.obs_dim} / {env.info.action_dim}")
        if not sigma > 0.0 or int(steps) < 1:
            raise _native.PbgError("EvolutionStrategy: sigma must be > 0 and steps >= 1")
        self.env, self.population = env, population
        self.sigma, self.lr, self.steps, self.seed = float(sigma), float(lr), int(steps), int(seed)
        self.init_q = None
        if init_q is not None:
            self.init_q = torch.as_tensor(init_q).to(device=env.device, dtype=torch.float32).contiguous()
        self.theta = population.init_theta(self.seed)
        self.generation = 0
        P, kw = population.n_members, dict(device=population.device)
        self.fitness = torch.zeros(P, dtype=torch.float64, **kw)   # of the last generation's members
        self._centred = torch.arange(P, dtype=torch.float32, **kw) / (P - 1) - 0.5
        self._ranks = torch.zeros(P, dtype=torch.float32, **kw)
        self._g = torch.zeros(population.n_params, dtype=torch.float32, **kw)
        self.obs_stats, self.obs_clip = None, float(obs_clip)
        if obs_norm:
            from .policy import ObsStats
            self.obs_stats = ObsStats(population.obs_dim, env.num_envs, group=env.num_envs // P, device=population.device)
            population.set_obs_norm(*self.obs_stats.finalize(), clip=self.obs_clip)  # the initial totals' normaliser

    def _rollout(self):
        self.env.reset(init_q=self.init_q)
        return self.env.rollout(self.population, self.steps, fresh=True)

    def step(self):
        """One generation; returns the members' fitness (a device tensor this object owns and overwrites)."""
        pop, gen = self.population, self.generation
        self.env.reset(init_q=self.init_q)
        pop.perturb(self.theta, self.sigma, self.seed, gen)
        if self.obs_stats is not None:
            pop.attach_obs_stats(self.obs_stats)
        res = self.env.rollout(pop, self.steps, fresh=True)
        if self.obs_stats is not None:
            pop.attach_obs_stats(None)
            pop.set_obs_norm(*self.obs_stats.finalize(), clip=self.obs_clip)
        self.update(res, gen)
        self.generation = gen + 1
        return self.fitness

    def update(self, res, generation: int):
        """The part of a generation after the rollout: fitness of ``res`` -> centred ranks -> gradient
        estimate -> ``theta`` moves.  ``generation`` must be the one the members were perturbed with."""
        pop, gen = self.population, int(generation)
        pop.fitness(res, out=self.fitness)
        # centred ranks in [-0.5, 0.5]; a NaN fitness (an env that blew up) ranks last, ties by member index
        fit = torch.where(torch.isnan(self.fitness), torch.full_like(self.fitness, float("-inf")), self.fitness)
        self._ranks[torch.argsort(fit, stable=True)] = self._centred
        w = (self._ranks[0::2] - self._ranks[1::2]).contiguous()
        pop.grad(w, self.seed, gen, out=self._g)
        self.theta.add_(self._g, alpha=self.lr / (pop.n_pairs * self.sigma))

    def evaluate(self):
        """Every member = the centre, one rollout: per-env ``(returns float64 [n], lengths int32 [n])``
        (of the first episode with ``autoreset=False``), fresh tensors."""
        self.population.set_all(self.theta)
        attached = self.population.obs_stats
        if attached is not None:
            self.population.attach_obs_stats(None)  # evaluating does not move the statistics
        res = self._rollout()
        if attached is not None:
            self.population.attach_obs_stats(attached)
        return res.done_return + res.cur_return, res.done_length + res.cur_length
