"""Tables of the camera renderer (include/render/rp_render.h), built from the generic `Model` (model/compile.py).

The renderer has a blob of its own (`make_render_blob`); the engine's model blob is not touched.  What is rendered
is what the engine knows: the key boxes, the piano base, the hands' COLLISION geoms (boxes, capsules, cylinders,
convex hulls, spheres) and the stage's floor.  The stand-in hand has no visual meshes.

Colours are this project's data, restated with their sources:
  keys / base   robopianist/models/piano/piano_constants.py:83-85
  fingertips    robopianist/models/hands/shadow_hand_constants.py:42-49 (FINGERTIP_COLORS), applied by
                robopianist/suite/tasks/piano_with_shadow_hands.py:121-122,451-460 when the task colourises
  floor         robopianist/models/arenas/stage.py:61-68: a plane of half-size 1 at z = 0 (its checker texture,
                rgb 0.1 / 0.2, is rendered as one 0.15 grey)
  lights        stage.py:37-40
"""

from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from robopianist_amd.model import compile as mcompile
from robopianist_amd.model import piano as piano_model
from robopianist_amd.model import shadow_hand, spec

WHITE_KEY_COLOR = (0.9, 0.9, 0.9)      # piano_constants.py:83
BLACK_KEY_COLOR = (0.1, 0.1, 0.1)      # piano_constants.py:84
BASE_COLOR = (0.15, 0.15, 0.15)        # piano_constants.py:85
HAND_COLOR = (0.5, 0.5, 0.5)           # one grey for every hand geom (MuJoCo's default geom rgba)
FLOOR_COLOR = (0.15, 0.15, 0.15)
BACKGROUND_COLOR = (0.1, 0.1, 0.1)
ACTIVATION_COLOR = (0.2, 0.8, 0.2)     # models/piano/piano.py:28
# shadow_hand_constants.py:42-49, in fingertip order th, ff, mf, rf, lf
FINGERTIP_COLORS = ((0.8, 0.2, 0.8), (0.8, 0.2, 0.2), (0.2, 0.8, 0.8), (0.2, 0.2, 0.8), (0.8, 0.8, 0.2))
FLOOR_HALF_SIZE = 1.0                  # stage.py:64
LIGHT_POSITIONS = ((0.0, 0.0, 1.0), (0.3, 0.0, 1.0))   # stage.py:37-40

# geoms are sorted by type in this order (every per-type loop of the kernel runs over one contiguous range)
TYPE_ORDER = (spec.GEOM_BOX, spec.GEOM_CAPSULE, spec.GEOM_CYLINDER, spec.GEOM_SPHERE, spec.GEOM_MESH)

MAX_BODIES = 256      # rp_render_frames_kernel: one thread per body in one workgroup
MAX_GEOMS = 1024      # rp_render_kernel: the env's geom frames (48 bytes each) are staged in LDS

_COPLANAR = 1e-9      # facets of one hull whose (unit normal, offset) differ by less are one face


def bounding_radius(rbound):
    """Radius of the kernel's ray / bounding-sphere reject for a geom of bounding radius `rbound`: the reject runs in
    float32, and a little slack keeps it from rejecting a grazing ray that the exact test would accept."""
    return np.asarray(rbound, np.float64) * 1.001 + 1e-5


def hull_planes(vertices: np.ndarray) -> np.ndarray:
    """Face planes [n][4] = (nx, ny, nz, d) with n.x <= d inside, unit normals, duplicate coplanar facets (qhull
    triangulates every face) merged."""
    try:
        from scipy.spatial import ConvexHull
    except ImportError as e:
        raise ImportError("the render tables need scipy (scipy.spatial.ConvexHull) to turn the hulls of GEOM_MESH "
                          "geoms into face planes") from e
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    eq = ConvexHull(v).equations          # [nfacet][4]: n.x + off <= 0 inside, unit n
    planes = []
    for n0, n1, n2, off in eq:
        p = np.array([n0, n1, n2, -off])
        if not any(np.abs(p - q).max() < _COPLANAR for q in planes):
            planes.append(p)
    return np.asarray(planes, np.float64)


def _top_level_ancestor(m, b: int) -> int:
    while int(m.body_parentid[b]) != 0:
        b = int(m.body_parentid[b])
    return b


def hand_root_bodies(m, key_joint_ids) -> np.ndarray:
    """Root body (child of the world) of every hand tree, in the order of RP_TREE_OFFSET's second index: the trees of
    the non-key dofs, ascending tree id (model/engine_tables.py)."""
    key_set = set(int(j) for j in key_joint_ids)
    first_dof = {}
    for j in range(int(m.nv)):
        if j not in key_set:
            first_dof.setdefault(int(m.dof_treeid[j]), j)
    return np.asarray([_top_level_ancestor(m, int(m.jnt_bodyid[first_dof[t]])) for t in sorted(first_dof)], np.int32)


def fingertip_body_ids(m) -> list:
    """[(body id, finger index 0-4)] of the fingertip bodies of every hand in the model."""
    out = []
    for b, name in enumerate(m.names["body"]):
        leaf = name.split("/")[-1]
        for i, f in enumerate(shadow_hand.FINGERTIP_BODIES):
            if leaf in ("rh_" + f, "lh_" + f):
                out.append((b, i))
    return out


def build_render_tables(m: mcompile.Model, key_joint_ids: Sequence[int], key_geom_ids: Sequence[int],
                        colorize_fingertips: bool = False) -> Dict[str, np.ndarray]:
    nb, ngeom = int(m.nbody), int(m.ngeom)
    if nb > MAX_BODIES:
        raise ValueError(f"the renderer walks the body tree in one workgroup: {nb} bodies > {MAX_BODIES}")
    if ngeom > MAX_GEOMS:
        raise ValueError(f"the renderer stages the geom frames in LDS: {ngeom} geoms > {MAX_GEOMS}")
    t: Dict[str, np.ndarray] = {}
    # ---- body tree --------------------------------------------------------------------------------------------
    level = np.zeros(nb, np.int32)
    for b in range(1, nb):
        assert int(m.body_parentid[b]) < b
        level[b] = level[int(m.body_parentid[b])] + 1
    for j in range(int(m.njnt)):
        if int(m.jnt_type[j]) not in (spec.JNT_HINGE, spec.JNT_SLIDE):
            raise ValueError(f"joint {j}: the renderer's kinematics cover hinge and slide joints only")
    roots = hand_root_bodies(m, key_joint_ids)
    body_tree = np.full(nb, -1, np.int32)
    body_tree[roots] = np.arange(len(roots), dtype=np.int32)
    t["rnd_nbody"] = np.array([nb], np.int32)
    t["rnd_nlevel"] = np.array([int(level.max(initial=0)) + 1], np.int32)
    t["rnd_body_parentid"] = np.asarray(m.body_parentid, np.int32)
    t["rnd_body_level"] = level
    t["rnd_body_pos"] = np.asarray(m.body_pos, np.float64)
    t["rnd_body_quat"] = np.asarray(m.body_quat, np.float64)
    t["rnd_body_jntadr"] = np.asarray(m.body_jntadr, np.int32)
    t["rnd_body_jntnum"] = np.asarray(m.body_jntnum, np.int32)
    t["rnd_body_tree"] = body_tree                       # index into tree_offset[env][.], -1 = not a hand root
    t["rnd_hand_root"] = roots
    t["rnd_ntree"] = np.array([len(roots)], np.int32)
    t["rnd_njnt"] = np.array([int(m.njnt)], np.int32)
    t["rnd_nv"] = np.array([int(m.nv)], np.int32)
    t["rnd_jnt_type"] = np.asarray(m.jnt_type, np.int32)
    t["rnd_jnt_axis"] = np.asarray(m.jnt_axis, np.float64).reshape(-1, 3)
    t["rnd_jnt_pos"] = np.asarray(m.jnt_pos, np.float64).reshape(-1, 3)
    t["rnd_jnt_qposadr"] = np.arange(int(m.njnt), dtype=np.int32)   # 1-dof joints: qpos address == joint id
    t["rnd_jnt_qpos0"] = np.asarray(m.qpos0, np.float64)
    # ---- geoms, sorted by type (stable: model order within a type) --------------------------------------------
    gtype = np.asarray(m.geom_type, np.int32)
    for g in range(ngeom):
        if int(gtype[g]) not in TYPE_ORDER:
            raise ValueError(f"geom {g}: type {int(gtype[g])} is not rendered")
    rank = np.array([TYPE_ORDER.index(int(x)) for x in gtype], np.int64)
    order = np.argsort(rank, kind="stable").astype(np.int32)
    rgb = np.tile(np.asarray(HAND_COLOR), (ngeom, 1))
    geom_key = np.full(ngeom, -1, np.int32)
    for k, g in enumerate(key_geom_ids):
        geom_key[int(g)] = k
        rgb[int(g)] = BLACK_KEY_COLOR if piano_model.is_key_black(k) else WHITE_KEY_COLOR
    names = m.names["geom"]
    for g in range(ngeom):
        if names[g] == "piano/base_geom":
            rgb[g] = BASE_COLOR
    if colorize_fingertips:
        tips = dict(fingertip_body_ids(m))
        for g in range(ngeom):
            if int(m.geom_bodyid[g]) in tips:
                rgb[g] = FINGERTIP_COLORS[tips[int(m.geom_bodyid[g])]]
    planes, cache = [], {}
    planeadr = np.full(ngeom, -1, np.int32); planenum = np.zeros(ngeom, np.int32)
    nplane = 0
    for g in range(ngeom):
        if int(gtype[g]) != spec.GEOM_MESH:
            continue
        a, n = int(m.geom_vertadr[g]), int(m.geom_vertnum[g])
        v = np.asarray(m.mesh_vert, np.float64).reshape(-1, 3)[a:a + n]
        key = v.tobytes()
        if key not in cache:                       # identical vertex sets share one plane list
            p = hull_planes(v)
            cache[key] = (nplane, len(p))
            planes.append(p); nplane += len(p)
        planeadr[g], planenum[g] = cache[key]
    mat = np.stack([spec.quat_to_mat(q) for q in np.asarray(m.geom_quat).reshape(-1, 4)]) if ngeom else np.zeros((0, 3, 3))
    t["rnd_ngeom"] = np.array([ngeom], np.int32)
    t["rnd_geom_id"] = order                                        # model geom id of sorted geom i
    t["rnd_geom_type"] = gtype[order]
    t["rnd_geom_bodyid"] = np.asarray(m.geom_bodyid, np.int32)[order]
    t["rnd_geom_pos"] = np.asarray(m.geom_pos, np.float64).reshape(-1, 3)[order]
    t["rnd_geom_mat"] = mat[order].reshape(-1, 9)
    t["rnd_geom_size"] = np.asarray(m.geom_size, np.float64).reshape(-1, 3)[order]
    t["rnd_geom_rbound"] = bounding_radius(np.asarray(m.geom_rbound, np.float64)[order])
    t["rnd_geom_rgb"] = rgb[order]
    t["rnd_geom_key"] = geom_key[order]
    t["rnd_geom_planeadr"] = planeadr[order]
    t["rnd_geom_planenum"] = planenum[order]
    t["rnd_nplane"] = np.array([nplane], np.int32)
    t["rnd_planes"] = np.concatenate(planes, 0) if planes else np.zeros((0, 4))
    ends = np.cumsum([int((rank == k).sum()) for k in range(len(TYPE_ORDER))]).astype(np.int32)
    t["rnd_type_end"] = ends                                        # end of each type's range in sorted order
    t["rnd_nkey"] = np.array([len(key_geom_ids)], np.int32)
    t["rnd_floor"] = np.array([FLOOR_HALF_SIZE, *FLOOR_COLOR], np.float64)
    t["rnd_background"] = np.asarray(BACKGROUND_COLOR, np.float64)
    t["rnd_lights"] = np.asarray(LIGHT_POSITIONS, np.float64).reshape(-1)
    return t


def make_render_blob(m: mcompile.Model, key_joint_ids, key_geom_ids, colorize_fingertips: bool = False,
                     tables=None) -> bytes:
    """The renderer's own blob (what rp_render_create expects): the container format of the model blob
    (model/compile.py: to_blob) holding the `rnd_*` tables only.  `tables`: the result of build_render_tables for the
    same arguments, when the caller has it already."""
    if tables is None:
        tables = build_render_tables(m, key_joint_ids, key_geom_ids, colorize_fingertips)
    head = mcompile.Model({k: m[k] for k in mcompile._SCALARS_I + mcompile._SCALARS_F})
    return mcompile.to_blob(head, extra=tables)
