"""ctypes binding of the camera renderer's C ABI (include/render/rp_render.h, librp_render.so).

`Renderer` renders one camera view of a batch of environments from the engine's qpos array, on the caller's HIP
stream, into torch tensors it caches per image size.  What it draws is the scene's collision geometry (model/
render_tables.py).  Like the engine, it has no CPU fallback: a missing library is an error.
"""

from __future__ import annotations

import ctypes

import numpy as np

from robopianist_amd import _abi
from robopianist_amd.model import cameras, render_tables

EXPORTED_SYMBOLS = ("rp_render_create", "rp_render_destroy", "rp_render", "rp_render_geom_frames", "rp_render_dim",
                    "rp_render_last_error")


class RenderError(RuntimeError):
    pass


class RenderArgs(ctypes.Structure):
    """rp_render_args (include/render/rp_render.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("qpos", ctypes.c_void_p),
        ("tree_offset", ctypes.c_void_p),
        ("key_rgb", ctypes.c_void_p),
        ("cam_pos", ctypes.c_double * 3),
        ("cam_rot", ctypes.c_double * 9),
        ("fovy_deg", ctypes.c_double),
        ("height", ctypes.c_int), ("width", ctypes.c_int),
        ("env_first", ctypes.c_int), ("env_count", ctypes.c_int),
        ("rgb", ctypes.c_void_p),
        ("depth", ctypes.c_void_p),
        ("segmentation", ctypes.c_void_p),
        ("hip_stream", ctypes.c_void_p),
    ]


def make_args(camera, height, width, env_first, env_count, qpos=None, tree_offset=None, key_rgb=None, rgb=None,
              depth=None, segmentation=None, hip_stream=None) -> RenderArgs:
    """Fills an rp_render_args; the array arguments are raw addresses (or None)."""
    cam = cameras.resolve(camera)
    return _abi.fill(RenderArgs, qpos=qpos, tree_offset=tree_offset, key_rgb=key_rgb,
                     cam_pos=(ctypes.c_double * 3)(*[float(x) for x in cam.pos]),
                     cam_rot=(ctypes.c_double * 9)(*[float(x) for x in np.asarray(cam.rot).reshape(-1)]),
                     fovy_deg=float(cam.fovy), height=int(height), width=int(width), env_first=int(env_first),
                     env_count=int(env_count), rgb=rgb, depth=depth, segmentation=segmentation, hip_stream=hip_stream)


_table = _abi.HandleTable("rp_render_", {"": RenderArgs}, RenderError, "RP_RENDER_LIB", "librp_render.so", "render",
                          create=[ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int],
                          extra={"geom_frames": [ctypes.c_void_p]})
LIB_PATH = _table.path
load_library, declare = _table.load, _table.declare


class Renderer(_abi.Owner):
    """Batched camera renderer of one compiled scene (`scene_info`: model/scene.py SceneInfo)."""

    def __init__(self, scene_info, n_envs: int, device_id: int = 0, precision: int = 64,
                 colorize_fingertips: bool = False):
        m = scene_info.model
        self.model = m
        self.n_envs, self.device_id, self.precision = int(n_envs), int(device_id), int(precision)
        self.piano_size = scene_info.piano_size
        tables = render_tables.build_render_tables(m, scene_info.key_joint_ids, scene_info.key_geom_ids,
                                                   colorize_fingertips=colorize_fingertips)
        self.blob = render_tables.make_render_blob(m, scene_info.key_joint_ids, scene_info.key_geom_ids,
                                                   colorize_fingertips=colorize_fingertips, tables=tables)
        self._handle = _abi.Handle(_table, self.blob, len(self.blob), self.n_envs, self.device_id, self.precision)
        self.ngeom, self.ntree = self._handle.dim("ngeom"), self._handle.dim("ntree")
        self.geom_id = np.asarray(tables["rnd_geom_id"], np.int64)   # model geom id of the renderer's geom i
        self._out = {}

    def outputs(self, height: int, width: int):
        """The cached output tensors of this image size: (rgb uint8 [E,H,W,3], depth float32 [E,H,W],
        segmentation int32 [E,H,W]), allocated at the first call."""
        import torch
        key = (int(height), int(width))
        if key not in self._out:
            dev = torch.device("cuda", self.device_id)
            E = self.n_envs
            self._out[key] = (torch.zeros((E,) + key + (3,), dtype=torch.uint8, device=dev),
                              torch.zeros((E,) + key, dtype=torch.float32, device=dev),
                              torch.zeros((E,) + key, dtype=torch.int32, device=dev))
        return self._out[key]

    def render_raw(self, args: RenderArgs) -> int:
        """rp_render with a caller-made argument block; returns the C return code (see last_error())."""
        return self._handle.call_raw("", args)

    def render(self, qpos, height: int, width: int, camera=-1, tree_offset=None, key_rgb=None, rgb=True,
               depth=False, segmentation=False, env_first: int = 0, env_count=None, hip_stream=None):
        """qpos / tree_offset / key_rgb: contiguous device tensors ([E,nv] and [E,ntree,3] of the renderer's
        precision, [E,88,3] uint8).  Returns (rgb, depth, segmentation): the cached output tensors of the
        requested outputs, None for the others.  Enqueues on `hip_stream` (default: torch's current stream)."""
        import torch
        if hip_stream is None:
            hip_stream = torch.cuda.current_stream(torch.device("cuda", self.device_id)).cuda_stream
        for t, shape in ((qpos, (self.n_envs, int(self.model.nv))), (tree_offset, (self.n_envs, self.ntree, 3)),
                         (key_rgb, (self.n_envs, 88, 3))):
            if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda):
                raise RenderError(f"render: expected a contiguous device tensor of shape {shape}, got {tuple(t.shape)}")
        if key_rgb is not None and key_rgb.dtype != torch.uint8:
            raise RenderError("render: key_rgb must be uint8")
        want = torch.float32 if self.precision == 32 else torch.float64
        for t in (qpos, tree_offset):
            if t is not None and t.dtype != want:
                raise RenderError(f"render: qpos / tree_offset must be {want}")
        o_rgb, o_depth, o_seg = self.outputs(height, width) if height > 0 and width > 0 else (None, None, None)
        cam = cameras.resolve(camera, self.piano_size)
        self._handle.call("", make_args(
            cam, height, width, env_first, self.n_envs - env_first if env_count is None else env_count,
            qpos=qpos.data_ptr() if qpos is not None else None,
            tree_offset=tree_offset.data_ptr() if tree_offset is not None else None,
            key_rgb=key_rgb.data_ptr() if key_rgb is not None else None,
            rgb=o_rgb.data_ptr() if (rgb and o_rgb is not None) else None,
            depth=o_depth.data_ptr() if (depth and o_depth is not None) else None,
            segmentation=o_seg.data_ptr() if (segmentation and o_seg is not None) else None, hip_stream=hip_stream))
        return (o_rgb if rgb else None, o_depth if depth else None, o_seg if segmentation else None)

    def geom_frames(self) -> np.ndarray:
        """Test seam (rp_render_geom_frames): (xpos [E,ngeom,3], xmat [E,ngeom,9]) of the last render as float32,
        indexed by MODEL geom id."""
        raw = np.zeros((self.n_envs, self.ngeom, 12), np.float32)
        if self._L.rp_render_geom_frames(self._h, raw.ctypes.data) != 0:
            raise RenderError(self.last_error())
        out = np.zeros_like(raw)
        out[:, self.geom_id] = raw
        return out[..., :3], out[..., 3:]
