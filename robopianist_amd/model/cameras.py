"""Cameras of the piano scene, restated as data.

  fixed cameras  robopianist/models/piano/piano.py:100-141 ("closeup", "left", "right", "back", "egocentric",
                 "topdown"), ids 0-5 in that order (the order MuJoCo numbers them in: the piano is the first entity
                 attached to the arena and the hands define none)
  free camera    robopianist/models/arenas/stage.py:27-30 (statistic.center / extent, global azimuth / elevation),
                 id -1 as in dm_control's `physics.render(camera_id=-1)`

A camera is (pos[3], rot[3x3], fovy in degrees); the columns of `rot` are the camera's x (right), y (up) and z (backwards:
the camera looks along -z) axes in world coordinates, MuJoCo's convention.
"""

from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from robopianist_amd.model import piano as piano_model
from robopianist_amd.model import spec

DEFAULT_FOVY = 45.0  # MuJoCo's default <camera fovy>


class Camera(NamedTuple):
    pos: np.ndarray    # [3]
    rot: np.ndarray    # [3][3], columns = camera x, y, z axes in the world frame
    fovy: float        # degrees


def rot_from_xyaxes(xyaxes) -> np.ndarray:
    """MuJoCo's `xyaxes` attribute: x normalised, y orthogonalised against x, z = x cross y."""
    a = np.asarray(xyaxes, np.float64)
    x = a[:3] / np.linalg.norm(a[:3])
    y = a[3:] - x * np.dot(x, a[3:])
    y = y / np.linalg.norm(y)
    return np.stack([x, y, np.cross(x, y)], axis=1)


# piano.py:102-131: name, pos, xyaxes
_XYAXES_CAMERAS = (
    ("closeup", (-0.313, 0.024, 0.455), (0.003, -1.000, -0.000, 0.607, 0.002, 0.795)),
    ("left", (0.393, -0.791, 0.638), (0.808, 0.589, 0.000, -0.388, 0.533, 0.752)),
    ("right", (0.472, 0.598, 0.580), (-0.637, 0.771, -0.000, -0.510, -0.421, 0.750)),
    ("back", (-0.569, 0.008, 0.841), (-0.009, -1.000, 0.000, 0.783, -0.007, 0.622)),
    ("egocentric", (0.417, -0.039, 0.717), (-0.002, 1.000, 0.000, -0.867, -0.002, 0.498)),
)
# piano.py:132-141: pad_y = 0.5, distance = 1.0, fovy = 2 atan2(pad_y * piano_size[1], distance), quat (1, 0, 0, 1)
_TOPDOWN_PAD_Y = 0.5
_TOPDOWN_DISTANCE = 1.0
_TOPDOWN_QUAT = (1.0, 0.0, 0.0, 1.0)

CAMERA_NAMES = tuple(c[0] for c in _XYAXES_CAMERAS) + ("topdown",)

# stage.py:27-30
FREE_LOOKAT = (0.2, 0.0, 0.3)
FREE_EXTENT = 0.6
FREE_AZIMUTH = 180.0
FREE_ELEVATION = -50.0
# Restated from memory of MuJoCo's mjv_defaultFreeCamera: the free camera starts 1.5 x the model's extent away from
# its look-at point (statistic.center).
FREE_DISTANCE_PER_EXTENT = 1.5


def topdown_fovy(piano_size=piano_model.BASE_SIZE) -> float:
    return math.degrees(2.0 * math.atan2(_TOPDOWN_PAD_Y * piano_size[1], _TOPDOWN_DISTANCE))


def fixed_cameras(piano_size=piano_model.BASE_SIZE):
    """The six piano cameras, in id order."""
    cams = [Camera(np.asarray(p, np.float64), rot_from_xyaxes(a), DEFAULT_FOVY) for _, p, a in _XYAXES_CAMERAS]
    cams.append(Camera(np.array([0.0, 0.0, _TOPDOWN_DISTANCE]), spec.quat_to_mat(_TOPDOWN_QUAT),
                       topdown_fovy(piano_size)))
    return cams


def free_camera() -> Camera:
    """The free camera's initial pose: looks at FREE_LOOKAT from `distance` away along the direction azimuth /
    elevation give (MuJoCo: forward = (cos e cos a, cos e sin a, sin e), right = forward x world z projected to the
    ground plane)."""
    az, el = math.radians(FREE_AZIMUTH), math.radians(FREE_ELEVATION)
    forward = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    right = np.array([math.sin(az), -math.cos(az), 0.0])
    up = np.cross(right, forward)
    dist = FREE_DISTANCE_PER_EXTENT * FREE_EXTENT
    pos = np.asarray(FREE_LOOKAT) - dist * forward
    return Camera(pos, np.stack([right, up, -forward], axis=1), DEFAULT_FOVY)


def resolve(camera, piano_size=piano_model.BASE_SIZE) -> Camera:
    """camera: an id (-1 = free camera, 0-5 fixed), a name ("back" or "piano/back"), or (pos[3], rot[3x3], fovy)."""
    if isinstance(camera, str):
        name = camera[len("piano/"):] if camera.startswith("piano/") else camera
        if name not in CAMERA_NAMES:
            raise ValueError(f"Unknown camera {camera!r}; cameras: {['piano/' + n for n in CAMERA_NAMES]}")
        return fixed_cameras(piano_size)[CAMERA_NAMES.index(name)]
    if isinstance(camera, (int, np.integer)):
        if camera == -1:
            return free_camera()
        if not 0 <= camera < len(CAMERA_NAMES):
            raise ValueError(f"camera_id {camera} out of range [-1, {len(CAMERA_NAMES)})")
        return fixed_cameras(piano_size)[int(camera)]
    try:
        pos, rot, fovy = camera
        pos = np.asarray(pos, np.float64).reshape(3)
        rot = np.asarray(rot, np.float64).reshape(3, 3)
        fovy = float(fovy)
    except (TypeError, ValueError) as e:
        raise ValueError("a camera is an id, a name or (pos[3], rot[3x3], fovy_deg)") from e
    if not 0.0 < fovy < 180.0:
        raise ValueError(f"fovy must be in (0, 180) degrees, got {fovy}")
    return Camera(pos, rot, fovy)
