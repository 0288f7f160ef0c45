"""PixelWrapper: adds the camera image of every env to the observation (robopianist/wrappers/pixels.py, built there
on dm_control's `physics.render`; here on the batched HIP renderer, include/render/rp_render.h)."""

from __future__ import annotations

import collections
from typing import Any, Dict, Optional

import numpy as np
import torch

from robopianist_amd.suite import specs

# the renderer's three outputs: rgb, depth, segmentation
_OUTPUT_DTYPES = {torch.uint8: np.dtype(np.uint8), torch.float32: np.dtype(np.float32), torch.int32: np.dtype(np.int32)}


class PixelWrapper:
    """`render_kwargs` are the keyword arguments of `TorchPhysics.render` (height, width, camera_id, depth,
    segmentation); the wrapped observation mapping gains `observation_key`: a device tensor [E,H,W,3] uint8 (or
    [E,H,W] with depth / segmentation).  The key colours of the task (`task.key_rgb`) and its fingertip colours are
    passed to the renderer.  The tensor is the renderer's cached buffer: it is overwritten by the next render."""

    def __init__(self, environment, render_kwargs: Optional[Dict[str, Any]] = None, observation_key: str = "pixels"):
        self._environment = environment
        self._render_kwargs = dict(render_kwargs or {})
        self._observation_key = observation_key
        wrapped = environment.observation_spec()
        if observation_key in wrapped:
            raise ValueError(f"observation key {observation_key!r} is already part of the wrapped observation")
        self._observation_spec = collections.OrderedDict(wrapped)
        pixels = self._render()   # the spec is extended from one render at construction
        self._observation_spec[observation_key] = specs.Array(
            tuple(pixels.shape[1:]), _OUTPUT_DTYPES[pixels.dtype], name=observation_key)

    def __getattr__(self, name):
        return getattr(self._environment, name)

    def _render(self):
        env = self._environment
        task, physics = env.task, env.physics
        kw = dict(self._render_kwargs)
        if hasattr(task, "key_rgb"):
            kw.setdefault("key_rgb", task.key_rgb(physics))
            kw.setdefault("colorize_fingertips", bool(getattr(task, "colorize_fingertips", False)))
        return physics.render(**kw)

    def _add_pixels(self, timestep):
        obs = collections.OrderedDict(timestep.observation)
        obs[self._observation_key] = self._render()
        return timestep._replace(observation=obs)

    def observation_spec(self):
        return self._observation_spec

    def reset(self):
        return self._add_pixels(self._environment.reset())

    def step(self, action):
        return self._add_pixels(self._environment.step(action))
