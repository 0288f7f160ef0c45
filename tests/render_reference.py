"""Shared helpers of the renderer's tests (tests/test_render_host.py, tests/test_gpu_render.py).

  * `reference_render`: an analytic numpy ray caster written from the image definition of include/render/rp_render.h,
    evaluated in float64 (the reference) or float32 (its own rounding error, from which the depth tolerance comes).
    It shares no code with csrc/rp_render.hpp: shapes are cut as unions / intersections of half spaces, balls and
    infinite cylinders, geom poses come from the CPU oracle's forward kinematics.
  * `HostRenderer`: csrc/rp_render.hpp compiled for the HOST with g++ into a temp dir (test infrastructure only: not
    built by build(), never loaded by the package).
  * the image cases (scenes, poses, cameras, size) and `compare_images`, the acceptance rule both suites use.

Depth tolerance.  `measure_reference_rounding()` renders every case with the reference in float32 and float64; the
largest depth difference on pixels where both see the same geom was 5.4969e-05 (scene "hull", camera topdown; the
other eleven images: 0.7e-05 .. 4.4e-05).  DEPTH_TOL = 4 x that = 2.1988e-04: the kernel's operation order and
-ffp-contract=on differ from numpy's.  The same evaluation gives the reference's own segmentation disagreement: at most
0.2273 % of an image (3 pixels of 1320: scene "cylinder", camera topdown; back: 0.0758 %, closeup and free: none), under
a quarter of the 1 % cap on every camera, so the 30 x 44 images and the cameras back / closeup / free / topdown are used
as they are (no yawed camera and no other size were needed).

The wide cases (`wide_cases`, `mixed_batch`) are judged by the SAME two figures.  The same evaluation over them gives a
depth rounding of at most 4.2014e-05 (scene "capsule", topdown, 32 x 40) and a segmentation disagreement of at most
0.1515 % (two pixels of 1320, mixed batch); tests/test_render_host.py asserts both per case, so a case that would need a
wider bound cannot be added: it has to move to another size or pose (two did, see _WIDE_SPEC and LOOK_AT_CAMERAS).
"""
import ctypes
import os
import subprocess
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W = 30, 44                      # H * W = 1320 is no multiple of 256: the last workgroup of an image is partial
CAMERAS = ("back", "closeup", -1, "topdown")
SCENES = ("capsule", "hull", "cylinder")
SEG_CAP = 0.01                     # at most 1 % of an image may differ in segmentation (and only next to a silhouette)
MEASURED_DEPTH_ROUNDING = 5.4969e-05
DEPTH_TOL = 4 * MEASURED_DEPTH_ROUNDING

_scene_cache = {}


def build_scene_variant(name):
    from robopianist_amd.model import scene
    if name not in _scene_cache:
        kw = {"capsule": dict(primitive_fingertip_collisions=True),
              "hull": dict(primitive_fingertip_collisions=False),
              "cylinder": dict(primitive_fingertip_collisions=True, cylinder_colliders=True)}[name]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _scene_cache[name] = scene.build_scene(gravity_compensation=True, **kw)
    return _scene_cache[name]


def random_pose(m, seed):
    """Joint angles drawn uniformly inside their ranges."""
    rng = np.random.default_rng(seed)
    lo, hi = m.jnt_range[:, 0], m.jnt_range[:, 1]
    q = lo + rng.uniform(0.05, 0.95, m.nv) * (hi - lo)
    return np.where(m.jnt_limited > 0, q, rng.uniform(-0.1, 0.1, m.nv))


def oracle_geom_poses(si, qpos, root_offsets=None):
    """(geom_xpos [ngeom,3], geom_xmat [ngeom,9]) of the oracle's forward kinematics at qpos.  root_offsets:
    {body id: xyz} added to body_pos of those bodies (how the oracle sees RP_TREE_OFFSET)."""
    from robopianist_amd import engine
    from oracle.rp_oracle import Oracle
    m = si.model
    orc = Oracle(m, engine.make_blob(m, si.key_joint_ids))
    for b, off in (root_offsets or {}).items():
        orc.body_pos[3 * b:3 * b + 3] += np.asarray(off, float)
    orc.reset()
    orc.qpos[:] = qpos
    orc.forward()
    return orc.geom_xpos.reshape(-1, 3).copy(), orc.geom_xmat.reshape(-1, 9).copy()


# ---------------------------------------------------------------------------------------------------------------
# the numpy reference
# ---------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _halfspaces(o, d, planes, f):
    """Interval of the ray inside the intersection of half spaces n.x <= c: (t0, t1, n0, n1, hit)."""
    P = o.shape[0]
    t0 = np.full(P, -np.inf, f); t1 = np.full(P, np.inf, f)
    n0 = np.zeros((P, 3), f); n1 = np.zeros((P, 3), f)
    ok = np.ones(P, bool)
    for pl in planes:
        n = pl[:3].astype(f); c = f(pl[3])
        den = _dot(d, n[None, :]); num = c - _dot(o, n[None, :])
        par = den == 0
        ok &= ~(par & (num < 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num / den
        ent = (den < 0) & (t > t0)
        t0 = np.where(ent, t, t0); n0 = np.where(ent[:, None], n[None, :], n0)
        ext = (den > 0) & (t < t1)
        t1 = np.where(ext, t, t1); n1 = np.where(ext[:, None], n[None, :], n1)
    return t0, t1, n0, n1, ok & (t0 <= t1)


def _ball(o, d, centre, r, f):
    oc = o - centre[None, :].astype(f)
    a = _dot(d, d); b = _dot(oc, d); c = _dot(oc, oc) - f(r) * f(r)
    disc = b * b - a * c
    hit = disc >= 0
    sq = np.sqrt(np.where(hit, disc, 0)).astype(f)
    t0 = (-b - sq) / a; t1 = (-b + sq) / a
    n0 = (oc + t0[:, None] * d) / f(r); n1 = (oc + t1[:, None] * d) / f(r)
    return t0, t1, n0, n1, hit


def _tube(o, d, r, f):
    """Infinite cylinder of radius r about z."""
    P = o.shape[0]
    a = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    b = o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]
    c = o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] - f(r) * f(r)
    par = a == 0
    disc = b * b - a * c
    hit = np.where(par, c <= 0, disc >= 0)
    sq = np.sqrt(np.where(disc >= 0, disc, 0)).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = np.where(par, -np.inf, (-b - sq) / a).astype(f); t1 = np.where(par, np.inf, (-b + sq) / a).astype(f)
    z = np.zeros(P, f)
    with np.errstate(invalid="ignore"):
        n0 = np.stack([(o[:, 0] + t0 * d[:, 0]) / f(r), (o[:, 1] + t0 * d[:, 1]) / f(r), z], 1)
        n1 = np.stack([(o[:, 0] + t1 * d[:, 0]) / f(r), (o[:, 1] + t1 * d[:, 1]) / f(r), z], 1)
    return t0, t1, np.nan_to_num(n0), np.nan_to_num(n1), hit


def _intersect(A, B):
    t0 = np.where(A[0] >= B[0], A[0], B[0]); n0 = np.where((A[0] >= B[0])[:, None], A[2], B[2])
    t1 = np.where(A[1] <= B[1], A[1], B[1]); n1 = np.where((A[1] <= B[1])[:, None], A[3], B[3])
    return t0, t1, n0, n1, A[4] & B[4] & (t0 <= t1)


def _convex_union(parts, f):
    """Interval of a CONVEX union of shapes: from the first entry to the last exit among the parts that are hit."""
    P = parts[0][0].shape[0]
    t0 = np.full(P, np.inf, f); t1 = np.full(P, -np.inf, f)
    n0 = np.zeros((P, 3), f); n1 = np.zeros((P, 3), f)
    hit = np.zeros(P, bool)
    for a0, a1, m0, m1, h in parts:
        e = h & (a0 < t0); t0 = np.where(e, a0, t0); n0 = np.where(e[:, None], m0, n0)
        x = h & (a1 > t1); t1 = np.where(x, a1, t1); n1 = np.where(x[:, None], m1, n1)
        hit |= h
    return t0, t1, n0, n1, hit


def _box_planes(s):
    return [np.array([sg if k == i else 0 for k in range(3)] + [s[i]], float) for i in range(3) for sg in (1.0, -1.0)]


def shape_span(gtype, size, planes, o, d, f):
    """(t0, t1, n0, n1, hit) of rays (o, d) [P,3] in the geom frame."""
    from robopianist_amd.model import spec
    if gtype == spec.GEOM_BOX:
        return _halfspaces(o, d, _box_planes(size), f)
    if gtype == spec.GEOM_MESH:
        return _halfspaces(o, d, planes, f)
    if gtype == spec.GEOM_SPHERE:
        return _ball(o, d, np.zeros(3), size[0], f)
    r, h = size[0], size[1]
    caps = _halfspaces(o, d, [np.array([0, 0, 1.0, h]), np.array([0, 0, -1.0, h])], f)
    cyl = _intersect(_tube(o, d, r, f), caps)
    if gtype == spec.GEOM_CYLINDER:
        return cyl
    assert gtype == spec.GEOM_CAPSULE
    return _convex_union([cyl, _ball(o, d, np.array([0, 0, h]), r, f), _ball(o, d, np.array([0, 0, -h]), r, f)], f)


def hull_planes_reference(m, g):
    from scipy.spatial import ConvexHull
    a, n = int(m.geom_vertadr[g]), int(m.geom_vertnum[g])
    eq = ConvexHull(np.asarray(m.mesh_vert).reshape(-1, 3)[a:a + n]).equations
    return np.concatenate([eq[:, :3], -eq[:, 3:]], 1)


def pixel_rays(cam, height, width, f):
    from robopianist_amd.model import cameras
    cam = cameras.resolve(cam)
    r, c = np.mgrid[0:height, 0:width]
    r = r.reshape(-1).astype(f); c = c.reshape(-1).astype(f)
    th = f(np.tan(0.5 * np.radians(cam.fovy)))
    x = (f(2) * (c + f(0.5)) / f(width) - f(1)) * th * (f(width) / f(height))
    y = (f(1) - f(2) * (r + f(0.5)) / f(height)) * th
    R = np.asarray(cam.rot, float).astype(f)
    d = np.stack([R[i, 0] * x + R[i, 1] * y - R[i, 2] for i in range(3)], 1)
    o = np.tile(np.asarray(cam.pos, float).astype(f)[None, :], (len(x), 1))
    return o, d


def geom_colours(si, colorize_fingertips=False):
    """Base colour of every model geom, from the documented rule (not from the render tables)."""
    from robopianist_amd.model import piano, render_tables as rt
    m = si.model
    col = np.tile(np.asarray(rt.HAND_COLOR), (m.ngeom, 1))
    for k, g in enumerate(si.key_geom_ids):
        col[g] = rt.BLACK_KEY_COLOR if piano.is_key_black(k) else rt.WHITE_KEY_COLOR
    col[m.names["geom"].index("piano/base_geom")] = rt.BASE_COLOR
    if colorize_fingertips:
        for b, i in rt.fingertip_body_ids(m):
            col[np.asarray(m.geom_bodyid) == b] = rt.FINGERTIP_COLORS[i]
    return col


def reference_render(si, xpos, xmat, cam, height=H, width=W, dtype=np.float64, key_rgb=None, colorize_fingertips=False,
                     stats=None):
    """Returns (rgb uint8 [H,W,3], depth float32-valued [H,W] of `dtype`, segmentation int32 [H,W]).  stats: an optional
    dict that receives "exit_pixels", the number of pixels whose visible hit is a shape's EXIT (the camera, or the ray's
    origin, lies inside that shape)."""
    from robopianist_amd.model import spec, render_tables as rt
    f = dtype
    m = si.model
    o, d = pixel_rays(cam, height, width, f)
    P = o.shape[0]
    best_t = np.full(P, np.inf, f); best_id = np.full(P, -1, np.int32); best_n = np.zeros((P, 3), f)
    best_exit = np.zeros(P, bool)
    col = geom_colours(si, colorize_fingertips)
    if key_rgb is not None:
        col[np.asarray(si.key_geom_ids)] = np.asarray(key_rgb, float) / 255.0
    plane_cache = {}
    for g in range(m.ngeom):
        R = np.asarray(xmat[g], float).reshape(3, 3).astype(f); p = np.asarray(xpos[g], float).astype(f)
        oc = o - p[None, :]
        ol = np.stack([R[0, i] * oc[:, 0] + R[1, i] * oc[:, 1] + R[2, i] * oc[:, 2] for i in range(3)], 1)
        dl = np.stack([R[0, i] * d[:, 0] + R[1, i] * d[:, 1] + R[2, i] * d[:, 2] for i in range(3)], 1)
        planes = None
        if int(m.geom_type[g]) == spec.GEOM_MESH:
            key = (int(m.geom_vertadr[g]), int(m.geom_vertnum[g]))
            if key not in plane_cache:
                plane_cache[key] = hull_planes_reference(m, g)
            planes = plane_cache[key]
        t0, t1, n0, n1, hit = shape_span(int(m.geom_type[g]), np.asarray(m.geom_size[g], float), planes, ol, dl, f)
        vis = hit & (t1 > 0)
        entry = t0 >= 0
        t = np.where(entry, t0, t1); n = np.where(entry[:, None], n0, n1)
        better = vis & (t < best_t)          # ascending model id: a later geom needs a strictly nearer hit
        nw = np.stack([R[i, 0] * n[:, 0] + R[i, 1] * n[:, 1] + R[i, 2] * n[:, 2] for i in range(3)], 1)
        best_t = np.where(better, t, best_t); best_id = np.where(better, g, best_id)
        best_n = np.where(better[:, None], nw, best_n)
        best_exit = np.where(better, ~entry, best_exit)
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = -o[:, 2] / d[:, 2]
        x = o[:, 0] + tf * d[:, 0]; y = o[:, 1] + tf * d[:, 1]
        fl = (d[:, 2] != 0) & (tf > 0) & (tf < best_t) & (np.abs(x) <= rt.FLOOR_HALF_SIZE) & (np.abs(y) <= rt.FLOOR_HALF_SIZE)
    best_t = np.where(fl, tf, best_t); best_id = np.where(fl, m.ngeom, best_id)
    best_n = np.where(fl[:, None], np.array([0, 0, 1], f)[None, :], best_n)
    if stats is not None:
        stats["exit_pixels"] = int((best_exit & ~fl).sum())
    colour = np.concatenate([col, [rt.FLOOR_COLOR], [rt.BACKGROUND_COLOR]], 0).astype(f)[best_id]   # (-1 = the last row)
    hitp = o + np.where(np.isfinite(best_t), best_t, 0)[:, None] * d
    shade = np.full(P, 0.4, f)
    for L in rt.LIGHT_POSITIONS:
        l = np.asarray(L, float).astype(f)[None, :] - hitp
        with np.errstate(invalid="ignore"):      # (a background pixel of a camera AT a light: its shade is replaced below)
            l = l / np.sqrt(_dot(l, l))[:, None]
        shade = shade + f(0.3) * np.maximum(0, _dot(best_n, l))
    shade = np.where(best_id < 0, 1.0, shade).astype(f)
    rgb = np.floor(255 * np.clip(colour * shade[:, None], 0, 1) + 0.5).astype(np.uint8)
    return rgb.reshape(height, width, 3), best_t.reshape(height, width), best_id.astype(np.int32).reshape(height, width)


# ---------------------------------------------------------------------------------------------------------------
# acceptance rule
# ---------------------------------------------------------------------------------------------------------------
def silhouette_neighbourhood(seg):
    """Pixels whose 8-neighbourhood (or the pixel itself) lies on a silhouette of `seg`: a pixel with a differently
    labelled 8-neighbour."""
    Hh, Ww = seg.shape
    pad = np.pad(seg, 1, mode="edge")
    edge = np.zeros((Hh, Ww), bool)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            edge |= pad[1 + dr:1 + dr + Hh, 1 + dc:1 + dc + Ww] != seg
    pe = np.pad(edge, 1, mode="constant")
    near = np.zeros((Hh, Ww), bool)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            near |= pe[1 + dr:1 + dr + Hh, 1 + dc:1 + dc + Ww]
    return near


def compare_images(got, ref, depth_tol=DEPTH_TOL, label=""):
    """got / ref = (rgb, depth, seg).  Prints the figures, then asserts: segmentation equal except next to a
    reference silhouette and on at most SEG_CAP of the image; depth within depth_tol and rgb within one level
    wherever the ids agree."""
    g_rgb, g_d, g_s = (np.asarray(x) for x in got)
    r_rgb, r_d, r_s = (np.asarray(x) for x in ref)
    diff = g_s != r_s
    same = ~diff
    fin = same & np.isfinite(r_d)
    derr = float(np.abs(g_d[fin].astype(np.float64) - r_d[fin].astype(np.float64)).max()) if fin.any() else 0.0
    cerr = int(np.abs(g_rgb[same].astype(int) - r_rgb[same].astype(int)).max()) if same.any() else 0
    off_edge = int((diff & ~silhouette_neighbourhood(r_s)).sum())
    print(f"{label}: seg mismatches {int(diff.sum())}/{diff.size} ({off_edge} away from a silhouette), "
          f"max depth err {derr:.3e} (tol {depth_tol:.3e}), max rgb err {cerr}")
    assert off_edge == 0, f"{label}: {off_edge} segmentation mismatches away from any silhouette"
    assert diff.mean() <= SEG_CAP, f"{label}: {diff.mean():.4f} of the image differs in segmentation"
    assert np.array_equal(np.isinf(g_d[same]), np.isinf(r_d[same])), f"{label}: background depth is not +inf"
    assert derr <= depth_tol, f"{label}: depth error {derr:.3e} > {depth_tol:.3e}"
    assert cerr <= 1, f"{label}: rgb differs by {cerr} levels where the ids agree"


def image_cases():
    """[(scene name, pose name, qpos)] -- every scene at a random pose inside the joint ranges; cameras: CAMERAS."""
    return [(name, "random", random_pose(build_scene_variant(name).model, seed=11 + i)) for i, name in enumerate(SCENES)]


_ref_cache = {}


def _key_part(v):
    return v if v is None or isinstance(v, (str, int, bool)) else np.asarray(v).tobytes()


def _camera_key(cam):
    if isinstance(cam, (str, int, np.integer)):
        return str(cam)
    pos, rot, fovy = cam
    return np.concatenate([np.ravel(pos), np.ravel(rot), [fovy]]).astype(np.float64).tobytes()


def root_offsets(si, offsets):
    """{hand root body: xyz} of per-root offsets [ntree][3] (RP_TREE_OFFSET's order: right hand first), as
    oracle_geom_poses takes them."""
    from robopianist_amd.model import render_tables
    if offsets is None:
        return None
    roots = render_tables.hand_root_bodies(si.model, si.key_joint_ids)
    return {int(b): np.asarray(offsets, float)[i] for i, b in enumerate(roots)}


def _reference_entry(scene_name, qpos, cam, dtype, offsets, height, width, kw):
    key = (scene_name, qpos.tobytes(), _camera_key(cam), np.dtype(dtype).name, _key_part(offsets), int(height), int(width),
           tuple(sorted((k, _key_part(v)) for k, v in kw.items())))
    if key not in _ref_cache:
        si = build_scene_variant(scene_name)
        pk = (scene_name, qpos.tobytes(), _key_part(offsets))
        if pk not in _ref_cache:
            _ref_cache[pk] = oracle_geom_poses(si, qpos, root_offsets(si, offsets))
        xpos, xmat = _ref_cache[pk]
        stats = {}
        images = reference_render(si, xpos, xmat, cam, height=height, width=width, dtype=dtype, stats=stats, **kw)
        _ref_cache[key] = (images, stats)
    return _ref_cache[key]


def reference_for(scene_name, qpos, cam, dtype=np.float64, offsets=None, height=H, width=W, **kw):
    """The reference's (rgb, depth, segmentation) of one image, computed once per process.  offsets: per-root tree
    offsets [ntree][3] or None; kw: key_rgb, colorize_fingertips."""
    return _reference_entry(scene_name, qpos, cam, dtype, offsets, height, width, kw)[0]


def reference_stats_for(scene_name, qpos, cam, dtype=np.float64, offsets=None, height=H, width=W, **kw):
    """The `stats` dict reference_render filled for the same image."""
    return _reference_entry(scene_name, qpos, cam, dtype, offsets, height, width, kw)[1]


# ---------------------------------------------------------------------------------------------------------------
# the wide cases: sizes on and next to a workgroup boundary, exact zeros, hand-placed cameras, tree offsets
# ---------------------------------------------------------------------------------------------------------------
def look_at(pos, target, up=(0.0, 0.0, 1.0), fovy=45.0):
    """A (pos, rot, fovy) camera at `pos` that looks at `target`, its y axis as close to `up` as that allows."""
    pos = np.asarray(pos, np.float64)
    fwd = np.asarray(target, np.float64) - pos
    fwd = fwd / np.linalg.norm(fwd)
    x = np.cross(fwd, np.asarray(up, np.float64))
    x = x / np.linalg.norm(x)
    return (tuple(pos.tolist()), np.stack([x, np.cross(x, fwd), -fwd], axis=1), float(fovy))


# straight down from above the keyboard; the matrix holds exact zeros and ones, so at an odd size the centre row and
# the centre column of the image have a ray component that is exactly 0
DOWN_CAMERA = ((0.1, 0, 1.0), [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], 50.0)

LOOK_AT_CAMERAS = {
    "far_corner": look_at((2, 2, 1.5), (0, 0, 0), fovy=60),               # the floor's edge and background, depth to 4 m
    "below": look_at((0.3, 0.1, -0.5), (0, 0, 0.2)),                      # the floor and the shapes from underneath
    "away": look_at((0, 0, 1), (0, 0, 5), up=(0, 1, 0)),                  # nothing but background
    # low over the keyboard, in the gap between the two middle keys and 77 mm in front of the piano's base: inside no
    # shape, every hit an entry
    "beside_base": look_at((0, 0, 0.02), (0.3, 0, 0.1)),
    # INSIDE the piano's base box (x -0.177 .. -0.077, z 0 .. 0.04), looking forwards and 25 degrees up: every pixel is
    # an exit hit of the base, through its front face below and its top face above.  No shape reaches into the base, so
    # the base is all that a camera inside it can show; no ray leaves through the bottom face, which lies in the floor.
    "inside_base": look_at((-0.127, 0.1, 0.01), (-0.127 + np.cos(np.radians(25)), 0.1, 0.01 + np.sin(np.radians(25))), fovy=40),
    "narrow": look_at((-0.5, 0, 0.6), (0, 0, 0.05), fovy=3),
    "wide": look_at((-0.3, 0, 0.4), (0.2, 0, 0.05), fovy=150),
}
ODD_H, ODD_W = 29, 43


WIDE_OFFSETS = ((0.0, 0.02, -0.05), (0.03, -0.04, 0.02))                  # right hand root, left hand root
MAGENTA = (255, 0, 255)

# (id, scene, pose, offsets?, camera, H, W, key colours and fingertip colours?)
_WIDE_SPEC = (
    [(f"size-{cam}-{h}x{w}", "capsule", "random", False, cam, h, w, False)
     for cam in ("back", "topdown") for h, w in ((16, 16), (32, 40), (3, 171), (1, 1))]
    + [(f"down-{name}-{h}x{w}", name, "zero", False, "down", h, w, False) for name in SCENES for h, w in ((ODD_H, ODD_W), (15, 17))]
    # (far_corner: scene "capsule" at ITS random pose has one grazing pixel of a finger capsule 3 m away whose depth the
    #  reference rounds by 9.03e-05 at 29 x 43, over the figure on record; at scene "hull"'s pose, seed 12, it is 0.85e-05)
    + [(f"{cam}-{name}", name, "seed12" if cam == "far_corner" else "random", False, cam, ODD_H, ODD_W, False)
       for cam in LOOK_AT_CAMERAS for name in ("capsule", "hull")]
    + [(f"offset-{name}-{cam}", name, "offset", True, cam, H, W, name == "capsule" and cam == "back")
       for name in ("capsule", "hull") for cam in ("back", "topdown")])


def wide_case_ids():
    return [c[0] for c in _WIDE_SPEC]


def base_key_rgb(n_envs=None):
    """The keys' own colours as uint8 [88][3] (or [n_envs][88][3]): what key_rgb holds while no key is coloured."""
    from robopianist_amd.model import piano
    k = np.where(np.array([piano.is_key_black(i) for i in range(88)])[:, None], 26, 230).astype(np.uint8).repeat(3, 1)
    return k if n_envs is None else np.ascontiguousarray(np.broadcast_to(k, (n_envs, 88, 3)))


def most_visible_key(si, seg):
    return int(np.argmax([(seg == g).sum() for g in si.key_geom_ids]))


_wide_cache = []


def wide_cases():
    """[(scene, qpos, per-root offsets [2][3] or None, camera, H, W, key_rgb [88][3] or None, colorize_fingertips)],
    in the order of wide_case_ids()."""
    if not _wide_cache:
        for _, name, pose, with_off, cam, h, w, coloured in _WIDE_SPEC:
            si = build_scene_variant(name)
            m = si.model
            q = {"random": lambda: image_cases()[SCENES.index(name)][2], "zero": lambda: np.zeros(m.nv),
                 "seed12": lambda: random_pose(m, 12),
                 "offset": lambda: random_pose(m, 3)}[pose]()
            off = np.asarray(WIDE_OFFSETS, np.float64) if with_off else None
            camera = DOWN_CAMERA if cam == "down" else LOOK_AT_CAMERAS.get(cam, cam)
            krgb = None
            if coloured:
                krgb = base_key_rgb()
                krgb[most_visible_key(si, reference_for(name, q, camera, offsets=off, height=h, width=w)[2])] = MAGENTA
            _wide_cache.append((name, q, off, camera, h, w, krgb, coloured))
    return list(_wide_cache)


MIXED_ENVS = 5


def mixed_batch():
    """(qpos [5][nv], offsets [5][2][3], key_rgb [5][88][3]) of scene "capsule": every env its own pose, tree offsets
    and key colours (rendered from camera "back" with the fingertip colours on)."""
    m = build_scene_variant("capsule").model
    rng = np.random.default_rng(77)
    q = np.stack([random_pose(m, 40 + e) for e in range(MIXED_ENVS)])
    off = rng.uniform(-0.04, 0.04, (MIXED_ENVS, 2, 3))
    off[0] = 0.0
    return q, off, rng.integers(0, 256, (MIXED_ENVS, 88, 3)).astype(np.uint8)


def rounded_to_float32(x):
    """x as the fp32 engine holds it, back in float64: what the reference gets when it is compared with precision 32."""
    return None if x is None else np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def reference_rounding(r64, r32):
    """(largest depth difference where the ids agree, fraction of the image whose ids differ) of two evaluations."""
    same = (r64[2] == r32[2]) & np.isfinite(r64[1])
    dd = float(np.abs(r64[1][same] - r32[1][same].astype(np.float64)).max()) if same.any() else 0.0
    return dd, float((r64[2] != r32[2]).mean())


def measure_reference_rounding(verbose=True):
    """float32 vs float64 evaluation of the reference on exactly the test images: (largest depth difference where the
    ids agree, largest fraction of an image whose ids differ, per camera)."""
    worst_d, worst_s = 0.0, {}
    for name, _, q in image_cases():
        for cam in CAMERAS:
            r64 = reference_for(name, q, cam, np.float64); r32 = reference_for(name, q, cam, np.float32)
            same = (r64[2] == r32[2]) & np.isfinite(r64[1])
            dd = float(np.abs(r64[1][same] - r32[1][same].astype(np.float64)).max()) if same.any() else 0.0
            frac = float((r64[2] != r32[2]).mean())
            if verbose:
                print(f"reference f32 vs f64: scene {name:8s} camera {str(cam):8s} depth {dd:.4e} seg {100 * frac:.4f} %")
            worst_d = max(worst_d, dd); worst_s[str(cam)] = max(worst_s.get(str(cam), 0.0), frac)
    return worst_d, worst_s


# ---------------------------------------------------------------------------------------------------------------
# csrc/rp_render.hpp on the host
# ---------------------------------------------------------------------------------------------------------------
_HOST_SRC = r"""
#include "rp_render.hpp"
static thread_local std::string g_err;
struct host_renderer { RprTables tab; int n_envs, precision; std::vector<float> frames; };
extern "C" {
const char* rph_last_error() { return g_err.c_str(); }
int rph_create(const void* blob, size_t bytes, int n_envs, int precision, void** out) {
  host_renderer* r = new host_renderer();
  g_err = r->tab.parse(blob, bytes);
  if (!g_err.empty() || n_envs <= 0) { delete r; *out = nullptr; return -1; }
  r->n_envs = n_envs; r->precision = precision;
  r->frames.assign((size_t)n_envs * (r->tab.M.ngeom ? r->tab.M.ngeom : 1) * RPR_FRAME, 0.0f);
  *out = r;
  return 0;
}
void rph_destroy(void* p) { delete (host_renderer*)p; }
int rph_render(void* p, const rp_render_args* a) {
  host_renderer* r = (host_renderer*)p;
  g_err = rpr_render_host(r->tab, r->n_envs, r->precision, a, r->frames.data());
  return g_err.empty() ? 0 : -1;
}
int rph_geom_frames(void* p, float* dst) {
  host_renderer* r = (host_renderer*)p;
  memcpy(dst, r->frames.data(), sizeof(float) * r->frames.size());
  return 0;
}
// the slices rp_render cuts a call of env_count envs into: writes (first, count) pairs, returns their number
int rph_slices(int env_count, int* out, int cap) {
  int n = 0;
  for (int first = 0; first < env_count && n < cap; first += RPR_MAX_GRID_Y, n++) {
    out[2 * n] = first; out[2 * n + 1] = rpr_slice_count(env_count, first);
  }
  return n;
}
int rph_ngeom(void* p) { return ((host_renderer*)p)->tab.M.ngeom; }
// one shape at the origin of the world (or none: type < 0) and the floor square of half size `floor_half` (< 0: no
// floor) against one ray: out = t, nx, ny, nz; returns the segmentation id (0 = the shape, 1 = the floor, -1)
int rph_trace_one(int type, const float* size, float rbound, const float* planes, int nplane, float floor_half,
                  const float* o, const float* d, float* out) {
  RprModel M;
  memset(&M, 0, sizeof(M));
  const int zero = 0, np_ = nplane;
  const float frame[RPR_FRAME] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  M.ngeom = 1;   // (the floor's id, with or without the shape)
  for (int k = 0; k < RPR_NTYPE; k++) M.type_end[k] = (type >= 0 && k >= type) ? 1 : 0;
  M.floor_half = floor_half;
  M.geom_id = &zero; M.geom_planeadr = &zero; M.geom_planenum = &np_;
  M.geom_size = size; M.geom_rbound = &rbound; M.planes = planes;
  RprHit hit;
  rpr_trace(M, frame, o, d, hit);
  out[0] = hit.t; out[1] = hit.n[0]; out[2] = hit.n[1]; out[3] = hit.n[2];
  return hit.id;
}
}
"""

_host_lib = None
_host_dir = None


def host_library():
    """Compiles csrc/rp_render.hpp with g++ (once per process) and loads the result."""
    global _host_lib, _host_dir
    if _host_lib is None:
        from robopianist_amd import render
        _host_dir = tempfile.TemporaryDirectory(prefix="rp_render_host_")
        src = os.path.join(_host_dir.name, "rp_render_host.cpp")
        so = os.path.join(_host_dir.name, "librp_render_host.so")
        with open(src, "w") as fh:
            fh.write(_HOST_SRC)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "robopianist_amd", "csrc"), src, "-o", so])
        L = ctypes.CDLL(so)
        L.rph_last_error.restype = ctypes.c_char_p
        L.rph_create.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.rph_destroy.argtypes = [ctypes.c_void_p]; L.rph_destroy.restype = None
        L.rph_render.argtypes = [ctypes.c_void_p, ctypes.POINTER(render.RenderArgs)]
        L.rph_geom_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.rph_ngeom.argtypes = [ctypes.c_void_p]
        L.rph_slices.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.rph_trace_one.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_int,
                                    ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _host_lib = L
    return _host_lib


def trace_one(gtype, size, o, d, planes=None, floor_half=-1.0, rbound=None):
    """One ray against one shape through the host-compiled routine: (t, normal[3], id)."""
    L = host_library()
    size = np.asarray(list(size) + [0.0] * (3 - len(size)), np.float32)
    pl = np.ascontiguousarray(planes if planes is not None else np.zeros((1, 4)), np.float32)
    o = np.asarray(o, np.float32); d = np.asarray(d, np.float32)
    out = np.zeros(4, np.float32)
    if rbound is None:
        rbound = 10.0
    rid = L.rph_trace_one(int(gtype), size.ctypes.data, float(rbound), pl.ctypes.data,
                          0 if planes is None else len(pl), float(floor_half), o.ctypes.data, d.ctypes.data, out.ctypes.data)
    return float(out[0]), out[1:].copy(), rid


class HostRenderer:
    """The renderer's whole call on the CPU (rpr_render_host), numpy arrays in and out."""

    def __init__(self, si, n_envs, precision=64, colorize_fingertips=False):
        from robopianist_amd.model import render_tables
        self._L = host_library()
        self.si, self.n_envs, self.precision = si, n_envs, precision
        tables = render_tables.build_render_tables(si.model, si.key_joint_ids, si.key_geom_ids, colorize_fingertips)
        self.blob = render_tables.make_render_blob(si.model, si.key_joint_ids, si.key_geom_ids, colorize_fingertips, tables=tables)
        self._h = ctypes.c_void_p()
        if self._L.rph_create(self.blob, len(self.blob), n_envs, precision, ctypes.byref(self._h)) != 0:
            raise RuntimeError(self._L.rph_last_error().decode())
        self.ngeom = self._L.rph_ngeom(self._h)
        self.geom_id = np.asarray(tables["rnd_geom_id"])

    def __del__(self):
        try:
            self._L.rph_destroy(self._h)
        except Exception:
            pass

    def render(self, qpos, cam, height=H, width=W, tree_offset=None, key_rgb=None, env_first=0, env_count=None, out=None):
        from robopianist_amd import render
        dt = np.float32 if self.precision == 32 else np.float64
        E = self.n_envs
        q = np.ascontiguousarray(np.broadcast_to(np.asarray(qpos, dt), (E, self.si.model.nv)))
        off = None if tree_offset is None else np.ascontiguousarray(tree_offset, dt)
        kr = None if key_rgb is None else np.ascontiguousarray(key_rgb, np.uint8)
        if out is None:
            out = (np.zeros((E, height, width, 3), np.uint8), np.zeros((E, height, width), np.float32),
                   np.zeros((E, height, width), np.int32))
        a = render.make_args(cam, height, width, env_first, E - env_first if env_count is None else env_count,
                             qpos=q.ctypes.data, tree_offset=None if off is None else off.ctypes.data,
                             key_rgb=None if kr is None else kr.ctypes.data, rgb=out[0].ctypes.data,
                             depth=out[1].ctypes.data, segmentation=out[2].ctypes.data)
        if self._L.rph_render(self._h, ctypes.byref(a)) != 0:
            raise RuntimeError(self._L.rph_last_error().decode())
        return out

    def geom_frames(self):
        raw = np.zeros((self.n_envs, self.ngeom, 12), np.float32)
        self._L.rph_geom_frames(self._h, raw.ctypes.data)
        o = np.zeros_like(raw)
        o[:, self.geom_id] = raw
        return o[..., :3], o[..., 3:]
