"""Tables of the fingertip inverse kinematics (include/control/rp_ik.h), built from a compiled scene (model/scene.py).

The solver has a blob of its own (`make_ik_blob`, the container format of `make_render_blob`); the engine's model blob is
not touched.  Per hand (right before left) the tables hold, padded to the solver's fixed sizes:

  the bodies of the hand's tree in model order (parents first): parent, level, local pose, joints
  the hand's joints in that walk order, each with its column = its index in HandInfo.joint_ids (the dof order)
  per column: qpos address and range (-inf / +inf for an unlimited joint)
  per fingertip: body, local site position, bitmask of the columns above it in the tree
  per actuator (HandInfo.actuator_ids order): transmission terms (column, coefficient) and ctrlrange
  the hand root's index into the engine's tree_offset array
"""

from __future__ import annotations

from typing import Dict

import numpy as np

from robopianist_amd.model import compile as mcompile
from robopianist_amd.model import render_tables, spec

MAX_HANDS = 2
MAX_DOFS = 32        # one lane per dof column: half a wave per hand
MAX_BODIES = 32      # one lane per body in the tree walk
MAX_ACTUATORS = 32   # one lane per actuator in the transmission
MAX_TERMS = 4        # joints of one fixed tendon
N_TIPS = 5

HAND_ORDER = ("right", "left")


def hand_order(scene_info):
    """The scene's hands in tip / action order."""
    return [s for s in HAND_ORDER if s in scene_info.hands]


def build_ik_tables(scene_info) -> Dict[str, np.ndarray]:
    m = scene_info.model
    sides = hand_order(scene_info)
    if not sides:
        raise ValueError("the fingertip IK needs a scene with at least one hand")
    roots = [int(r) for r in render_tables.hand_root_bodies(m, scene_info.key_joint_ids)]
    H = MAX_HANDS
    hand_i = np.zeros((H, 8), np.int32)
    body_i = np.zeros((H, MAX_BODIES, 4), np.int32)
    body_d = np.zeros((H, MAX_BODIES, 7), np.float64); body_d[:, :, 3] = 1.0
    jnt_i = np.zeros((H, MAX_DOFS, 2), np.int32)
    jnt_d = np.zeros((H, MAX_DOFS, 6), np.float64)
    col_i = np.zeros((H, MAX_DOFS), np.int32)
    col_d = np.zeros((H, MAX_DOFS, 2), np.float64)
    tip_i = np.zeros((H, N_TIPS, 2), np.uint32)
    tip_d = np.zeros((H, N_TIPS, 3), np.float64)
    act_i = np.zeros((H, MAX_ACTUATORS, 1 + MAX_TERMS), np.int32)
    act_d = np.zeros((H, MAX_ACTUATORS, MAX_TERMS + 2), np.float64)
    qoff = aoff = 0
    for h, side in enumerate(sides):
        info = scene_info.hands[side]
        root = int(info.root_body_id)
        joint_ids = [int(j) for j in info.joint_ids]
        n = len(joint_ids)
        if n > MAX_DOFS:
            raise ValueError(f"{side} hand: {n} dofs > {MAX_DOFS} (the IK maps one lane to one dof of a hand)")
        if len(set(joint_ids)) != n:
            raise ValueError(f"{side} hand: joint_ids repeats a joint")
        col_of = {j: c for c, j in enumerate(joint_ids)}
        # ---- the hand's tree ----------------------------------------------------------------------------------
        local = {}
        for b in range(int(m.nbody)):
            if b == root or int(m.body_parentid[b]) in local:
                local[b] = len(local)
        if len(local) > MAX_BODIES:
            raise ValueError(f"{side} hand: {len(local)} bodies > {MAX_BODIES} (the IK walks the tree with one lane per body)")
        if int(m.body_parentid[root]) != 0:
            raise ValueError(f"{side} hand: the root body is not a child of the world")
        nj = 0
        for b, lb in local.items():
            par = -1 if b == root else local[int(m.body_parentid[b])]
            body_i[h, lb] = (par, 0 if par < 0 else body_i[h, par, 1] + 1, nj, int(m.body_jntnum[b]))
            body_d[h, lb, :3] = m.body_pos[b]
            body_d[h, lb, 3:] = m.body_quat[b]
            for j in range(int(m.body_jntadr[b]), int(m.body_jntadr[b]) + int(m.body_jntnum[b])):
                jt = int(m.jnt_type[j])
                if jt not in (spec.JNT_HINGE, spec.JNT_SLIDE):
                    raise ValueError(f"joint {j} ({m.names['joint'][j]}): the IK covers hinge and slide joints only")
                if j not in col_of:
                    raise ValueError(f"joint {j} ({m.names['joint'][j]}) moves the {side} hand but is not one of its joint_ids")
                if float(m.qpos0[j]) != 0.0:
                    raise ValueError(f"joint {j}: the IK expects qpos0 = 0")
                jnt_i[h, nj] = (jt, col_of[j])
                jnt_d[h, nj, :3] = m.jnt_axis[j]
                jnt_d[h, nj, 3:] = m.jnt_pos[j]
                nj += 1
        if nj != n:
            raise ValueError(f"{side} hand: {n - nj} of its joint_ids are not on the bodies of its tree")
        for c, j in enumerate(joint_ids):
            col_i[h, c] = j                                  # 1-dof joints: qpos address == joint id
            col_d[h, c] = m.jnt_range[j] if int(m.jnt_limited[j]) else (-np.inf, np.inf)
        # ---- fingertips ---------------------------------------------------------------------------------------
        sites = [int(s) for s in info.fingertip_site_ids]
        if len(sites) != N_TIPS:
            raise ValueError(f"{side} hand: {len(sites)} fingertip sites, expected {N_TIPS}")
        for i, s in enumerate(sites):
            b = int(m.site_bodyid[s])
            if b not in local:
                raise ValueError(f"fingertip site {s} is not on the {side} hand")
            mask, a = 0, b
            while a != 0:
                for j in range(int(m.body_jntadr[a]), int(m.body_jntadr[a]) + int(m.body_jntnum[a])):
                    mask |= 1 << col_of[j]
                a = int(m.body_parentid[a])
            tip_i[h, i] = (local[b], mask)
            tip_d[h, i] = m.site_pos[s]
        # ---- actuators ----------------------------------------------------------------------------------------
        acts = [int(a) for a in info.actuator_ids]
        if len(acts) > MAX_ACTUATORS:
            raise ValueError(f"{side} hand: {len(acts)} actuators > {MAX_ACTUATORS}")
        for k, a in enumerate(acts):
            name = m.names["actuator"][a]
            gain, bias = float(m.actuator_gainprm[a]), np.asarray(m.actuator_biasprm[a], np.float64)
            if float(m.actuator_gear[a]) != 1.0 or not gain > 0.0 or bias[0] != 0.0 or bias[1] != -gain or bias[2] != 0.0:
                raise ValueError(f"actuator {a} ({name}) is not a gear-1 position actuator: its ctrl is not a position target")
            tt, tid = int(m.actuator_trntype[a]), int(m.actuator_trnid[a])
            if tt == spec.TRN_JOINT:
                terms = [(tid, 1.0)]
            elif tt == spec.TRN_TENDON:
                w0, wn = int(m.tendon_adr[tid]), int(m.tendon_num[tid])
                terms = [(int(m.wrap_objid[w0 + i]), float(m.wrap_prm[w0 + i])) for i in range(wn)]
            else:
                raise ValueError(f"actuator {a} ({name}): transmission type {tt} is neither a joint nor a fixed tendon")
            if len(terms) > MAX_TERMS:
                raise ValueError(f"actuator {a} ({name}): a tendon of {len(terms)} joints > {MAX_TERMS}")
            for i, (j, coef) in enumerate(terms):
                if j not in col_of:
                    raise ValueError(f"actuator {a} ({name}) acts on joint {j}, outside its own ({side}) hand")
                act_i[h, k, 1 + i] = col_of[j]
                act_d[h, k, i] = coef
            act_i[h, k, 0] = len(terms)
            act_d[h, k, MAX_TERMS:] = m.actuator_ctrlrange[a] if int(m.actuator_ctrllimited[a]) else (-np.inf, np.inf)
        if root not in roots:
            raise ValueError(f"{side} hand: its root body is not one of the engine's hand trees")
        nlevel = int(body_i[h, :len(local), 1].max()) + 1
        hand_i[h] = (n, len(local), len(acts), nlevel, roots.index(root), qoff, aoff, 0)
        qoff += n
        aoff += len(acts)
    t: Dict[str, np.ndarray] = {}
    t["ik_dims"] = np.array([len(sides), int(m.nv), len(roots), int(hand_i[:, 3].max()), qoff, aoff, 0, 0], np.int32)
    t["ik_hand_i"] = hand_i
    t["ik_body_i"] = body_i
    t["ik_body_d"] = body_d
    t["ik_jnt_i"] = jnt_i
    t["ik_jnt_d"] = jnt_d
    t["ik_col_i"] = col_i
    t["ik_col_d"] = col_d
    t["ik_tip_i"] = tip_i.view(np.int32)     # (the column mask may use bit 31)
    t["ik_tip_d"] = tip_d
    t["ik_act_i"] = act_i
    t["ik_act_d"] = act_d
    return t


def make_ik_blob(scene_info, tables=None) -> bytes:
    """The solver's own blob (what rp_ik_create expects): the container format of the model blob (model/compile.py:
    to_blob) holding the `ik_*` tables only.  `tables`: the result of build_ik_tables, when the caller has it already."""
    if tables is None:
        tables = build_ik_tables(scene_info)
    m = scene_info.model
    head = mcompile.Model({k: m[k] for k in mcompile._SCALARS_I + mcompile._SCALARS_F})
    return mcompile.to_blob(head, extra=tables)
