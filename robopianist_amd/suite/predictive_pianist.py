"""PredictivePianist: the second pianist without training.  Every control step it plans (planning.PredictiveSampler:
K candidate action splines per env, rolled out H control steps in a K times larger planning environment, the best kept)
and steps the real environment with the winner's first action.

When both environments are FingertipActionWrappers in absolute mode it can be seeded: every step the plan's nominal is
set to FingeringPianist's action (the fingers the MIDI's fingering assigns aim at their keys) and the candidates are
perturbations of it, so the planner refines the first pianist instead of searching from nothing."""

from __future__ import annotations

import torch

from robopianist_amd import planning


class PredictivePianist:
    """`env`: the real environment (an Environment, or a FingertipActionWrapper); `make_env(n_envs)`: builds the planning
    environment with the same task arguments and the same wrapper.  `seed_from`: a FingeringPianist on `env` (needs the
    fingertip wrapper in absolute mode on both environments), or None.  The other arguments are PredictiveSampler's."""

    def __init__(self, env, make_env, n_candidates: int, horizon: int, n_knots: int = 2, spline: str = "linear",
                 sigma=0.1, gamma: float = 1.0, seed: int = 0, seed_from=None):
        self._env = env
        self._sampler = planning.PredictiveSampler(env, make_env, n_candidates, horizon, n_knots, spline=spline,
                                                   sigma=sigma, gamma=gamma, seed=seed)
        self._seed_from = seed_from
        if seed_from is not None:
            plan_env = self._sampler.plan_env
            if not (hasattr(env, "set_weights") and hasattr(plan_env, "set_weights")):
                raise ValueError("seed_from needs a FingertipActionWrapper on the real and on the planning environment")
            if getattr(env, "_mode", None) != "absolute" or getattr(plan_env, "_mode", None) != "absolute":
                raise ValueError("seed_from needs both FingertipActionWrappers in absolute mode (FingeringPianist's targets "
                                 "are world positions)")

    @property
    def sampler(self) -> planning.PredictiveSampler:
        return self._sampler

    def action(self):
        """The [G, nu] action for the step about to be taken (live: the next call overwrites it)."""
        s = self._sampler
        if self._seed_from is not None:
            a, weights = self._seed_from.action()
            # the tip weights are the wrapper's, not the action's: the candidates of a group plan under their env's
            self._env.set_weights(weights, validate=False)
            s.plan_env.set_weights(weights.repeat_interleave(s.K, dim=0), validate=False)
            s.set_nominal(a)
        return s.plan()

    def step(self):
        """Plans, then steps the real environment with the chosen action; returns its TimeStep."""
        return self._env.step(self.action())

    def play(self, max_steps=None):
        """Resets the real environment and plays until every env's episode has ended (or `max_steps`); returns
        (the return of every env [G], the number of control steps).  Reads one flag back per step."""
        ts = self._env.reset()
        ret = torch.zeros(self._env.n_envs, dtype=torch.float64, device=self._env.physics.device)
        done = torch.zeros_like(ret, dtype=torch.bool)
        steps = 0
        while max_steps is None or steps < max_steps:
            ts = self.step()
            ret += torch.where(done, torch.zeros_like(ret), ts.reward.to(torch.float64))
            done |= ts.last()
            steps += 1
            if bool(done.all()):
                break
        return ret, steps
