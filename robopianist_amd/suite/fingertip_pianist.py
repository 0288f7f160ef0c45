"""FingeringPianist: a pianist without training, for FingertipActionWrapper(mode="absolute").

The task knows which finger belongs on which key (the MIDI's fingering: `task._finger_next`) and where that key's target
lies (`task._key_targets`).  Every step, a finger the fingering assigns to a key of the coming goal aims at that key's
target, lowered by `press_depth`, with weight 1; every other finger has weight 0 and goes where the hand takes it.
Torch only, on the physics device, nothing is read back; the inverse kinematics that turns the targets into an action
is the wrapper's (include/control/rp_ik.h)."""

from __future__ import annotations

import torch


class FingeringPianist:
    """`env`: a FingertipActionWrapper (or the Environment below it) on a task with a fingering.  `press_depth`: metres
    below the key's target surface point to aim at, so that the key goes down.  `lead_steps` >= 1: how many control
    steps of the goal the fingers look ahead; 1 = the step about to be simulated (`task._finger_next`), larger values
    add the following steps' fingering, nearer steps winning a finger that is wanted twice.  A finger assigned to
    several keys of one step aims at the lowest of them."""

    def __init__(self, env, press_depth: float, lead_steps: int = 1):
        task = env.task
        if not hasattr(task, "_finger_next") or not hasattr(task, "_key_targets"):
            raise ValueError(f"FingeringPianist needs a task with a fingering ({type(task).__name__} has none)")
        if int(lead_steps) < 1:
            raise ValueError("lead_steps must be >= 1")
        self._env, self._task = env, task
        self._press_depth, self._lead = float(press_depth), int(lead_steps)
        self._n_tips = 5 * len(task.scene.hands)
        dev = env.physics.device
        self._tip_ids = torch.arange(self._n_tips, device=dev)
        self._key_ids = torch.arange(88, device=dev)

    @property
    def n_tips(self) -> int:
        return self._n_tips

    def _fingering(self, k: int):
        """[E, 88] tip index of every goal key `k` steps after the one about to be simulated, -1 = none."""
        task = self._task
        if k == 0:
            return task._finger_next
        slen = task._song_len[task._song_id]
        t = task._t_idx + k
        idx = torch.clamp(t, max=task._finger_bank.shape[1] - 1)
        f = task._finger_bank[task._song_id, idx]
        goal = (task._goal_bank[task._song_id, idx][:, :88] > 0) & (t < slen)[:, None]
        side = getattr(task, "hand_side", None)
        if side == "right":
            goal, f = goal & (f < 5), torch.where(f < 0, torch.full_like(f, 4), f)
        elif side == "left":
            goal, f = goal & (f >= 5), f - 5
        return torch.where(goal, f, torch.full_like(f, -1))

    def targets(self):
        """(targets [E, T, 3] float64 world positions, weights [E, T] float64) for the step about to be taken."""
        task, phys = self._task, self._env.physics
        key_targets = task._key_targets(phys).to(torch.float64)                  # [E, 88, 3]
        E = key_targets.shape[0]
        key = torch.full((E, self._n_tips), 88, device=key_targets.device, dtype=torch.long)
        for k in reversed(range(self._lead)):
            f = self._fingering(k)
            mine = f[:, :, None] == self._tip_ids[None, None, :]                  # [E, 88, T]
            first = torch.where(mine, self._key_ids[None, :, None], 88).amin(dim=1)
            key = torch.where(first < 88, first, key)
        has = key < 88
        pick = torch.clamp(key, max=87)[..., None].expand(-1, -1, 3)
        tg = torch.gather(key_targets, 1, pick).clone()
        tg[..., 2] -= self._press_depth
        tg = torch.where(has[..., None], tg, torch.zeros_like(tg))
        return tg.contiguous(), has.to(torch.float64)

    def action(self, sustain=None):
        """The wrapper's action [E, 3 T + 1] (absolute mode) and the weights to hand to `set_weights`."""
        tg, w = self.targets()
        E = tg.shape[0]
        s = torch.zeros((E, 1), dtype=tg.dtype, device=tg.device) if sustain is None else \
            torch.as_tensor(sustain, dtype=tg.dtype, device=tg.device).reshape(E, 1)
        return torch.cat([tg.reshape(E, -1), s], dim=1), w
