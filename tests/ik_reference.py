"""Reference side of the fingertip-IK tests (include/control/rp_ik.h): a numpy float64 twin of the definition, the cases
the CPU and the GPU tests share, and the g++ build of csrc/rp_ik.hpp.

The twin is written from the header's definition on the compiled MODEL (model/compile.py arrays), not on the solver's
tables and not after csrc/rp_ik.hpp: frames are rotation matrices (Rodrigues' formula per hinge) where the library
composes quaternions, the Jacobian is collected by walking up from every tip where the library masks columns, and the
damped system is handed to numpy's LU solve where the library factors A = L L^T.
"""

from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile
import warnings

import numpy as np

from robopianist_amd.model import scene as scene_lib
from robopianist_amd.model import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DAMPING, MAX_STEP = 0.03, 0.02

# Measured on the CPU (tests/test_ik_host.py's docstring says of what; its tests keep them honest): the tolerances are
# 4 x the measured maxima, and the CPU and the GPU tests share them.
MEASURED_JAC = 4.7e-12     # twin Jacobian vs central differences
MEASURED_CTRL = 2.9e-14    # g++ build vs twin, ctrl / q_target / residual, over CASES
MEASURED_TIP = 1.7e-16     # g++ build vs twin, tip positions, over CASES
JAC_TOL, CTRL_TOL, TIP_TOL = 4 * MEASURED_JAC, 4 * MEASURED_CTRL, 4 * MEASURED_TIP


# ---- the twin ---------------------------------------------------------------------------------------------------------
def hands_of(scene_info):
    return [scene_info.hands[s] for s in ("right", "left") if s in scene_info.hands]


def tree_index(scene_info, info):
    """Index of the hand into tree_offset[env]: the hand trees in ascending tree order, i.e. ascending root body."""
    roots = sorted(int(h.root_body_id) for h in scene_info.hands.values())
    return roots.index(int(info.root_body_id))


def _quat_mat(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _subtree(m, root):
    keep = []
    for b in range(int(m.nbody)):
        if b == root or int(m.body_parentid[b]) in keep:
            keep.append(b)
    return keep


def frames(m, info, q_hand, offset=None):
    """World frames of the hand's bodies and joints at the hand's dofs `q_hand` (HandInfo.joint_ids order).
    Returns (xpos {body: [3]}, xmat {body: [3,3]}, axis {joint: [3]}, anchor {joint: [3]})."""
    qof = {int(j): float(q_hand[c]) for c, j in enumerate(info.joint_ids)}
    root = int(info.root_body_id)
    xpos, xmat, axis, anchor = {0: np.zeros(3)}, {0: np.eye(3)}, {}, {}
    for b in _subtree(m, root):
        par = int(m.body_parentid[b])
        local = np.asarray(m.body_pos[b], np.float64) + (np.asarray(offset, np.float64) if (b == root and offset is not None) else 0.0)
        pos = xpos[par] + xmat[par] @ local
        mat = xmat[par] @ _quat_mat(m.body_quat[b])
        for j in range(int(m.body_jntadr[b]), int(m.body_jntadr[b]) + int(m.body_jntnum[b])):
            axis[j] = mat @ m.jnt_axis[j]
            anchor[j] = pos + mat @ m.jnt_pos[j]
            if int(m.jnt_type[j]) == spec.JNT_SLIDE:
                pos = pos + axis[j] * qof[j]
            else:
                mat = mat @ _rodrigues(m.jnt_axis[j], qof[j])
                pos = anchor[j] - mat @ m.jnt_pos[j]
        xpos[b], xmat[b] = pos, mat
    return xpos, xmat, axis, anchor


def fk(m, info, q_hand, offset=None):
    """World positions of the hand's five fingertips, [5, 3]."""
    xpos, xmat, _, _ = frames(m, info, q_hand, offset)
    return np.stack([xpos[int(m.site_bodyid[s])] + xmat[int(m.site_bodyid[s])] @ m.site_pos[s]
                     for s in info.fingertip_site_ids])


def jacobian(m, info, q_hand, offset=None):
    """Unweighted tip Jacobian [15, n] at `q_hand`, and the tips [5, 3]."""
    xpos, xmat, axis, anchor = frames(m, info, q_hand, offset)
    col = {int(j): c for c, j in enumerate(info.joint_ids)}
    J = np.zeros((15, len(info.joint_ids)))
    tips = np.zeros((5, 3))
    for i, s in enumerate(info.fingertip_site_ids):
        b = int(m.site_bodyid[s])
        tips[i] = xpos[b] + xmat[b] @ m.site_pos[s]
        while b != 0:
            for j in range(int(m.body_jntadr[b]), int(m.body_jntadr[b]) + int(m.body_jntnum[b])):
                J[3 * i:3 * i + 3, col[j]] = (axis[j] if int(m.jnt_type[j]) == spec.JNT_SLIDE
                                              else np.cross(axis[j], tips[i] - anchor[j]))
            b = int(m.body_parentid[b])
    return J, tips


def clamp_q(m, info, q):
    j = np.asarray(info.joint_ids)
    lim = np.asarray(m.jnt_limited)[j] != 0
    return np.where(lim, np.clip(q, m.jnt_range[j, 0], m.jnt_range[j, 1]), q)


def transmission(m, info, q_hand):
    """ctrl of the hand's actuators that holds q_hand: clamp(sum coef q, ctrlrange)."""
    col = {int(j): c for c, j in enumerate(info.joint_ids)}
    out = np.zeros(len(info.actuator_ids))
    for k, a in enumerate(info.actuator_ids):
        tid = int(m.actuator_trnid[a])
        if int(m.actuator_trntype[a]) == spec.TRN_JOINT:
            v = q_hand[col[tid]]
        else:
            w0, wn = int(m.tendon_adr[tid]), int(m.tendon_num[tid])
            v = sum(float(m.wrap_prm[w0 + i]) * q_hand[col[int(m.wrap_objid[w0 + i])]] for i in range(wn))
        if int(m.actuator_ctrllimited[a]):
            v = min(max(v, m.actuator_ctrlrange[a, 0]), m.actuator_ctrlrange[a, 1])
        out[k] = v
    return out


def solve_hand(m, info, q0, target, weight, delta, offset, damping, max_step, iterations, dof_weight=None):
    """One env, one hand.  Returns (ctrl [a], q^K [n], residual [5], tips(q^0) [5,3])."""
    q = np.array(q0, np.float64)
    D = np.ones(len(q)) if dof_weight is None else np.asarray(dof_weight, np.float64)
    w = np.asarray(weight, np.float64)
    goal = tips0 = None
    for it in range(iterations):
        J, tips = jacobian(m, info, q, offset)
        if it == 0:
            tips0 = tips.copy()
            goal = tips + target if delta else np.array(target, np.float64)
        d = goal - tips
        nrm = np.linalg.norm(d, axis=1)
        scale = np.where(nrm > max_step, max_step / np.where(nrm > 0, nrm, 1.0), 1.0)
        e = (w[:, None] * d * scale[:, None]).reshape(-1)
        Jw = J * np.repeat(w, 3)[:, None]
        A = (Jw * D[None, :]) @ Jw.T + damping ** 2 * np.eye(15)
        q = clamp_q(m, info, q + D * (Jw.T @ np.linalg.solve(A, e)))
    res = np.linalg.norm(goal - fk(m, info, q, offset), axis=1)
    return transmission(m, info, q), q, res, tips0


def solve(scene_info, qpos, targets, weights=None, delta=False, tree_offset=None, damping=DAMPING, max_step=MAX_STEP,
          iterations=1, dof_weight=None):
    """The whole call: dict(ctrl [E, A], q [E, sum n], residual [E, T], tips [E, T, 3])."""
    m = scene_info.model
    hs = hands_of(scene_info)
    qpos = np.asarray(qpos, np.float64)
    E, T = len(qpos), 5 * len(hs)
    targets = np.asarray(targets, np.float64).reshape(E, T, 3)
    weights = np.ones((E, T)) if weights is None else np.asarray(weights, np.float64).reshape(E, T)
    out = dict(ctrl=[], q=[], residual=[], tips=[])
    for e in range(E):
        rows, qo = dict(ctrl=[], q=[], residual=[], tips=[]), 0
        for h, info in enumerate(hs):
            n = len(info.joint_ids)
            off = None if tree_offset is None else np.asarray(tree_offset, np.float64)[e, tree_index(scene_info, info)]
            dw = None if dof_weight is None else np.asarray(dof_weight, np.float64)[qo:qo + n]
            c, q, r, t = solve_hand(m, info, qpos[e, info.joint_ids], targets[e, 5 * h:5 * h + 5], weights[e, 5 * h:5 * h + 5],
                                    delta, off, damping, max_step, iterations, dw)
            for k, v in zip(("ctrl", "q", "residual", "tips"), (c, q, r, t)):
                rows[k].append(v)
            qo += n
        for k in out:
            out[k].append(np.concatenate(rows[k], 0))
    return {k: np.stack(v) for k, v in out.items()}


# ---- scenes and cases ---------------------------------------------------------------------------------------------------
_scenes = {}

SCENES = {
    "two": dict(),
    "right": dict(hands=("right",)),
    "left": dict(hands=("left",)),
    "reduced": dict(reduced_action_space=True),
    "forearm6": dict(forearm_dofs=("forearm_tx", "forearm_ty", "forearm_tz", "forearm_roll", "forearm_pitch", "forearm_yaw")),
}


def scene(name):
    if name not in _scenes:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _scenes[name] = scene_lib.build_scene(primitive_fingertip_collisions=True, **SCENES[name])
    return _scenes[name]


def hand_ranges(si, info):
    m = si.model
    j = np.asarray(info.joint_ids)
    return m.jnt_range[j, 0].copy(), m.jnt_range[j, 1].copy()


def pose(si, rng, E, lo_frac=0.3, hi_frac=0.7):
    """qpos [E, nv]: every hand dof at lo_frac..hi_frac of its range, the keys at rest."""
    m = si.model
    q = np.zeros((E, int(m.nv)))
    for info in hands_of(si):
        lo, hi = hand_ranges(si, info)
        q[:, info.joint_ids] = lo + rng.uniform(lo_frac, hi_frac, (E, len(lo))) * (hi - lo)
    return q


def reachable_targets(si, rng, qpos, spread=0.15, tree_offset=None):
    """FK(q+) with q+ = clamp(q + U(-spread, spread) min(1, range)): [E, T, 3]."""
    m = si.model
    out = []
    for e in range(len(qpos)):
        row = []
        for info in hands_of(si):
            lo, hi = hand_ranges(si, info)
            qd = clamp_q(m, info, qpos[e, info.joint_ids] + rng.uniform(-spread, spread, len(lo)) * np.minimum(1.0, hi - lo))
            off = None if tree_offset is None else tree_offset[e, tree_index(si, info)]
            row.append(fk(m, info, qd, off))
        out.append(np.concatenate(row, 0))
    return np.stack(out)


def current_tips(si, qpos, tree_offset=None):
    m = si.model
    return np.stack([np.concatenate([fk(m, info, qpos[e, info.joint_ids],
                                        None if tree_offset is None else tree_offset[e, tree_index(si, info)])
                                     for info in hands_of(si)], 0) for e in range(len(qpos))])


def n_trees(si):
    return len(si.hands)


def make_case(name):
    """A shared parity case: dict(scene, qpos, targets, weights, delta, tree_offset, iterations, ...)."""
    spec_ = CASES[name]
    si = scene(spec_.get("scene", "two"))
    rng = np.random.default_rng(spec_.get("seed", 7))
    E = spec_.get("E", 3)
    T = 5 * len(si.hands)
    qpos = pose(si, rng, E)
    off = None
    if spec_.get("offset"):
        off = rng.uniform(-0.05, 0.05, (E, n_trees(si), 3))
    if spec_.get("on_limits"):
        for info in hands_of(si):
            lo, hi = hand_ranges(si, info)
            qpos[:, info.joint_ids] = np.where(rng.uniform(size=(E, len(lo))) < 0.5, lo, hi)
    delta = bool(spec_.get("delta", False))
    if spec_.get("far"):
        targets = current_tips(si, qpos, off) + 0.5 * np.stack([np.ones((E, T)), np.zeros((E, T)), np.ones((E, T))], -1) / np.sqrt(2.0)
        if delta:
            targets = targets - current_tips(si, qpos, off)
    elif delta:
        targets = rng.uniform(-0.02, 0.02, (E, T, 3))
    else:
        targets = reachable_targets(si, rng, qpos, tree_offset=off)
    weights = None
    if spec_.get("weights") == "mixed":
        weights = np.where(rng.uniform(size=(E, T)) < 0.4, 0.0, rng.uniform(0.2, 2.0, (E, T)))
        weights[0, 0], weights[0, 1] = 0.0, 1.0
    elif spec_.get("weights") == "zero":
        weights = np.zeros((E, T))
    return dict(name=name, scene=si, qpos=qpos, targets=targets, weights=weights, delta=delta, tree_offset=off,
                iterations=spec_.get("K", 1), damping=DAMPING, max_step=MAX_STEP, dof_weight=None)


# every GPU parity case; the CPU tests run the g++ build over the same list
CASES = {
    "two_k1":            dict(E=3),
    "two_k4":            dict(E=3, K=4),
    "two_e1_delta":      dict(E=1, delta=True, K=4),
    "two_e130":          dict(E=130, K=1, weights="mixed", seed=11),
    "right_only":        dict(scene="right", E=3, K=4),
    "left_only":         dict(scene="left", E=3, K=4, offset=True),
    "reduced":           dict(scene="reduced", E=3, K=4),
    "forearm6":          dict(scene="forearm6", E=3, K=4),
    "mixed_weights":     dict(E=3, K=4, weights="mixed"),
    "zero_weights":      dict(E=3, K=1, weights="zero"),
    "far_targets":       dict(E=3, K=4, far=True),
    "far_delta":         dict(E=3, K=1, far=True, delta=True),
    "on_limits":         dict(E=3, K=4, on_limits=True, far=True),
    "tree_offset":       dict(E=3, K=4, offset=True),
    "tree_offset_delta": dict(E=3, K=1, offset=True, delta=True),
}

_twin_cache = {}


def twin_of(name):
    """(case, the twin's result), computed once per process and shared; callers leave both unchanged."""
    if name not in _twin_cache:
        c = make_case(name)
        r = solve(c["scene"], c["qpos"], c["targets"], c["weights"], c["delta"], c["tree_offset"], c["damping"],
                  c["max_step"], c["iterations"], c["dof_weight"])
        for v in r.values():
            v.setflags(write=False)
        _twin_cache[name] = (c, r)
    return _twin_cache[name]


# ---- the g++ build of csrc/rp_ik.hpp ------------------------------------------------------------------------------------
_HOST_SRC = r"""
#include "rp_ik.hpp"
struct rp_ik { RpikModel M; int n_envs, precision; };
static thread_local std::string g_err;
extern "C" {
const char* rpikh_last_error(void) { return g_err.c_str(); }
int rpikh_create(const void* blob, size_t bytes, int n_envs, int device, int precision, rp_ik** out) {
  (void)device;
  rp_ik* r = new rp_ik();
  g_err = rpik_parse(blob, bytes, r->M);
  if (!g_err.empty() || n_envs <= 0 || (precision != 32 && precision != 64)) { delete r; *out = nullptr; return -1; }
  r->n_envs = n_envs; r->precision = precision; *out = r;
  return 0;
}
void rpikh_destroy(rp_ik* r) { delete r; }
int rpikh_solve(rp_ik* r, const rp_ik_args* a) { g_err = rpik_solve_host(r->M, a, r->n_envs, r->precision); return g_err.empty() ? 0 : -1; }
int rpikh_dim(const rp_ik* r, const char* name) {
  if (!strcmp(name, "n_act")) return r->M.nact;
  if (!strcmp(name, "n_dof")) return r->M.ndof;
  if (!strcmp(name, "n_tips")) return RPIK_TIPS * r->M.nhand;
  if (!strcmp(name, "ntree")) return r->M.ntree;
  return -1;
}
}
"""

# A stand-alone program for the sanitizer run: reads a blob and one call's arrays from files, solves, writes ctrl.
_SANITIZER_MAIN = r"""
#include <stdio.h>
#include <vector>
#include "rp_ik.hpp"
static std::vector<char> slurp(const char* path) {
  std::vector<char> v; FILE* f = fopen(path, "rb"); if (!f) return v;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); v.resize(n);
  if (n && fread(v.data(), 1, n, f) != (size_t)n) v.clear();
  fclose(f); return v;
}
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::vector<char> blob = slurp(argv[1]), in = slurp(argv[2]);
  RpikModel* M = new RpikModel();
  std::string err = rpik_parse(blob.data(), blob.size(), *M);
  if (!err.empty()) { fprintf(stderr, "%s\n", err.c_str()); return 3; }
  // input: int32 E, K, delta, has_offset; then float64 qpos [E][nv], offset [E][ntree][3], target [E][T][3], weight [E][T]
  const int* hd = (const int*)in.data();
  const int E = hd[0], K = hd[1], delta = hd[2], has_off = hd[3], T = RPIK_TIPS * M->nhand;
  const double* d = (const double*)(in.data() + 16);
  const size_t need = 16 + 8 * ((size_t)E * M->nv + (size_t)E * M->ntree * 3 + (size_t)E * T * 4);
  if (in.size() != need) { fprintf(stderr, "bad input size\n"); return 4; }
  // (exact-size heap arrays: an access past any of them is the sanitizer's to report)
  std::vector<double> qpos(d, d + (size_t)E * M->nv); d += (size_t)E * M->nv;
  std::vector<double> off(d, d + (size_t)E * M->ntree * 3); d += (size_t)E * M->ntree * 3;
  std::vector<double> target(d, d + (size_t)E * T * 3); d += (size_t)E * T * 3;
  std::vector<double> weight(d, d + (size_t)E * T);
  std::vector<double> out((size_t)E * M->nact), q((size_t)E * M->ndof), res((size_t)E * T), tips((size_t)E * T * 3);
  rp_ik_args a; memset(&a, 0, sizeof(a));
  a.struct_size = sizeof(a); a.qpos = qpos.data(); a.tree_offset = has_off ? off.data() : nullptr;
  a.target = target.data(); a.weight = weight.data(); a.delta = delta; a.iterations = K; a.lambda = 0.03; a.max_step = 0.02;
  a.out = out.data(); a.out_stride = M->nact; a.q_target = q.data(); a.residual = res.data(); a.tips = tips.data();
  a.env_first = 0; a.env_count = E;
  err = rpik_solve_host(*M, &a, E, 64);
  if (!err.empty()) { fprintf(stderr, "%s\n", err.c_str()); return 5; }
  FILE* f = fopen(argv[3], "wb"); if (!f) return 6;
  fwrite(out.data(), 8, out.size(), f); fclose(f);
  delete M;
  return 0;
}
"""

_host_lib = None
_host_dir = None


def host_dir():
    global _host_dir
    if _host_dir is None:
        _host_dir = tempfile.TemporaryDirectory(prefix="rp_ik_host_")
    return _host_dir.name


def host_library():
    """Compiles csrc/rp_ik.hpp with g++ (once per process) and loads the result."""
    global _host_lib
    if _host_lib is None:
        from robopianist_amd import kinematics
        src = os.path.join(host_dir(), "rp_ik_host.cpp")
        so = os.path.join(host_dir(), "librp_ik_host.so")
        with open(src, "w") as fh:
            fh.write(_HOST_SRC)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "robopianist_amd", "csrc"), src, "-o", so])
        _host_lib = kinematics.declare(ctypes.CDLL(so), "rpikh_")
    return _host_lib


def sanitizer_program():
    """Builds the stand-alone program with AddressSanitizer and UBSan, their runtimes linked statically (the program then
    runs the same whatever else the process loads first); returns its path."""
    src = os.path.join(host_dir(), "rp_ik_sanitize.cpp")
    exe = os.path.join(host_dir(), "rp_ik_sanitize")
    with open(src, "w") as fh:
        fh.write(_SANITIZER_MAIN)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "robopianist_amd", "csrc"), src, "-o", exe])
    return exe


class HostIK:
    """rp_ik_solve on the CPU (rpik_solve_host), numpy arrays in and out."""

    def __init__(self, scene_info, n_envs, precision=64, blob=None):
        from robopianist_amd.model import ik_tables
        self.L = host_library()
        self.blob = ik_tables.make_ik_blob(scene_info) if blob is None else blob
        self.h = ctypes.c_void_p()
        if self.L.rpikh_create(self.blob, len(self.blob), n_envs, 0, precision, ctypes.byref(self.h)) != 0:
            raise RuntimeError(self.L.rpikh_last_error().decode())
        self.E, self.precision = n_envs, precision
        self.dtype = np.float32 if precision == 32 else np.float64
        dim = lambda n: self.L.rpikh_dim(self.h, n)
        self.n_act, self.n_dof, self.n_tips, self.ntree = dim(b"n_act"), dim(b"n_dof"), dim(b"n_tips"), dim(b"ntree")

    def __del__(self):
        if getattr(self, "h", None):
            self.L.rpikh_destroy(self.h)
            self.h = None

    def solve(self, qpos, targets, weights=None, delta=False, tree_offset=None, damping=DAMPING, max_step=MAX_STEP,
              iterations=1, dof_weight=None, env_first=0, env_count=None, out=None, fill=None):
        from robopianist_amd import kinematics
        E = self.E
        qpos = np.ascontiguousarray(qpos, self.dtype)
        off = None if tree_offset is None else np.ascontiguousarray(tree_offset, self.dtype)
        tg = np.ascontiguousarray(targets, np.float64)
        w = None if weights is None else np.ascontiguousarray(weights, np.float64)
        dw = None if dof_weight is None else np.ascontiguousarray(dof_weight, np.float64)
        out = np.zeros((E, self.n_act), self.dtype) if out is None else out
        q = np.full((E, self.n_dof), np.nan if fill is None else fill)
        res = np.full((E, self.n_tips), np.nan if fill is None else fill)
        tips = np.full((E, self.n_tips, 3), np.nan if fill is None else fill)
        ptr = lambda a: None if a is None else a.ctypes.data
        a = kinematics.make_args(env_first, E - env_first if env_count is None else env_count, qpos=ptr(qpos),
                                 tree_offset=ptr(off), target=ptr(tg), weight=ptr(w), dof_weight=ptr(dw), delta=delta,
                                 damping=damping, max_step=max_step, iterations=iterations, out=ptr(out),
                                 out_stride=out.strides[0] // out.itemsize, q_target=ptr(q), residual=ptr(res), tips=ptr(tips))
        if self.L.rpikh_solve(self.h, ctypes.byref(a)) != 0:
            raise RuntimeError(self.L.rpikh_last_error().decode())
        return dict(ctrl=out, q=q, residual=res, tips=tips)


def host_of(name, precision=64):
    c, _ = twin_of(name)
    h = HostIK(c["scene"], len(c["qpos"]), precision)
    return h.solve(c["qpos"], c["targets"], c["weights"], c["delta"], c["tree_offset"], c["damping"], c["max_step"],
                   c["iterations"], c["dof_weight"])
