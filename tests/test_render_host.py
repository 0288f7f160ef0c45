"""CPU tests of the camera renderer (include/render/rp_render.h): tables, cameras, the per-ray routine of csrc/rp_render.hpp
compiled for the host, whole images against the numpy reference, and the key-colour rule.

Depth tolerance (tests/render_reference.py): the numpy reference evaluated in float32 against itself in float64 on
exactly these images differs by at most 5.4969e-05 in depth where the ids agree; DEPTH_TOL = 4 x that = 2.1988e-04.
Its own segmentation disagreement is at most 0.2273 % of an image (camera topdown), under a quarter of the 1 % cap on
every camera, so the images are 30 x 44 from the cameras back / closeup / free / topdown as they stand.
"""
import math

import numpy as np
import pytest
import torch

import render_reference as rr
from fake_physics import FakePhysics
from robopianist_amd import engine
from robopianist_amd.model import cameras, piano, render_tables, spec


# ---- tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.SCENES)
def test_render_tables(name):
    si = rr.build_scene_variant(name)
    m = si.model
    before = engine.make_blob(m, si.key_joint_ids)
    t = render_tables.build_render_tables(m, si.key_joint_ids, si.key_geom_ids)
    blob = render_tables.make_render_blob(m, si.key_joint_ids, si.key_geom_ids)
    assert engine.make_blob(m, si.key_joint_ids) == before, "building the render tables changed the engine's blob"
    assert blob != before and len(blob) < len(before)
    ids = t["rnd_geom_id"]
    assert sorted(ids.tolist()) == list(range(m.ngeom))
    rank = [render_tables.TYPE_ORDER.index(int(x)) for x in t["rnd_geom_type"]]
    assert rank == sorted(rank), "geoms are not sorted by type"
    assert np.array_equal(t["rnd_geom_type"], m.geom_type[ids])
    assert t["rnd_type_end"][-1] == m.ngeom
    # hull planes: every vertex inside every plane, every plane touches a face
    n_hulls = 0
    for i, g in enumerate(ids):
        if int(m.geom_type[g]) != spec.GEOM_MESH:
            continue
        n_hulls += 1
        v = m.mesh_vert[m.geom_vertadr[g]:m.geom_vertadr[g] + m.geom_vertnum[g]]
        pl = t["rnd_planes"][t["rnd_geom_planeadr"][i]:t["rnd_geom_planeadr"][i] + t["rnd_geom_planenum"][i]]
        assert len(pl) >= 4
        s = v @ pl[:, :3].T - pl[:, 3][None, :]          # [vertex][plane]
        assert s.max() <= 1e-12
        assert ((np.abs(s) <= 1e-12).sum(axis=0) >= 3).all(), "a plane touches fewer than three vertices"
        assert np.allclose(np.linalg.norm(pl[:, :3], axis=1), 1.0, atol=1e-12)
        # merged: no two planes of one hull coincide
        d = np.abs(pl[:, None, :] - pl[None, :, :]).max(-1) + np.eye(len(pl))
        assert d.min() > 1e-9
    assert n_hulls == (10 if name == "hull" else 0)
    if name == "hull":   # identical vertex sets share one plane list
        adr = t["rnd_geom_planeadr"][t["rnd_geom_type"] == spec.GEOM_MESH]
        assert len(set(adr.tolist())) < len(adr)
    # hand roots in the order of RP_TREE_OFFSET's second index (right hand first)
    roots = [m.names["body"][b] for b in t["rnd_hand_root"]]
    assert [r.split("/")[0] for r in roots] == ["rh_shadow_hand", "lh_shadow_hand"]
    assert all(m.body_parentid[b] == 0 for b in t["rnd_hand_root"])
    # colours
    rgb = np.zeros((m.ngeom, 3)); rgb[ids] = t["rnd_geom_rgb"]
    assert np.allclose(rgb[si.key_geom_ids[0]], 0.9) and np.allclose(rgb[si.key_geom_ids[1]], 0.1)
    assert np.allclose(rgb[m.names["geom"].index("piano/base_geom")], 0.15)
    tips = render_tables.build_render_tables(m, si.key_joint_ids, si.key_geom_ids, colorize_fingertips=True)
    rgb2 = np.zeros((m.ngeom, 3)); rgb2[ids] = tips["rnd_geom_rgb"]
    changed = np.flatnonzero(np.abs(rgb2 - rgb).max(1) > 0)
    tip_bodies = dict(render_tables.fingertip_body_ids(m))
    assert len(tip_bodies) == 10 and len(changed) >= 10
    for g in changed:
        assert np.allclose(rgb2[g], render_tables.FINGERTIP_COLORS[tip_bodies[int(m.geom_bodyid[g])]])


def test_render_tables_need_scipy_for_hulls(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError("no scipy")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(ImportError, match="scipy"):
        render_tables.hull_planes(np.random.default_rng(0).normal(size=(8, 3)))


# ---- cameras -----------------------------------------------------------------------------------------------------
def test_cameras():
    cams = cameras.fixed_cameras()
    assert cameras.CAMERA_NAMES == ("closeup", "left", "right", "back", "egocentric", "topdown")
    for c in cams + [cameras.free_camera()]:
        assert np.abs(c.rot.T @ c.rot - np.eye(3)).max() < 1e-12
        assert abs(np.linalg.det(c.rot) - 1) < 1e-12
    # the cited numbers (models/piano/piano.py:100-141)
    cited = {"closeup": ((-0.313, 0.024, 0.455), (0.003, -1.0, 0.0), (0.607, 0.002, 0.795)),
             "left": ((0.393, -0.791, 0.638), (0.808, 0.589, 0.0), (-0.388, 0.533, 0.752)),
             "right": ((0.472, 0.598, 0.580), (-0.637, 0.771, 0.0), (-0.510, -0.421, 0.750)),
             "back": ((-0.569, 0.008, 0.841), (-0.009, -1.0, 0.0), (0.783, -0.007, 0.622)),
             "egocentric": ((0.417, -0.039, 0.717), (-0.002, 1.0, 0.0), (-0.867, -0.002, 0.498))}
    for i, name in enumerate(cameras.CAMERA_NAMES[:5]):
        pos, x, y = (np.asarray(v) for v in cited[name])
        c = cameras.resolve(name)
        assert np.array_equal(c.pos, pos) and c.fovy == 45.0
        assert np.allclose(c.rot[:, 0], x / np.linalg.norm(x), atol=1e-15)
        yo = y - c.rot[:, 0] * (c.rot[:, 0] @ y)
        assert np.allclose(c.rot[:, 1], yo / np.linalg.norm(yo), atol=1e-15)
        assert np.allclose(c.rot[:, 2], np.cross(c.rot[:, 0], c.rot[:, 1]), atol=1e-15)
        assert np.abs(c.rot[:, 1] - y).max() < 2e-3      # (the cited y axes are orthogonal to x to three digits)
        for other in (i, "piano/" + name):
            o = cameras.resolve(other)
            assert np.array_equal(o.pos, c.pos) and np.array_equal(o.rot, c.rot) and o.fovy == c.fovy
    top = cameras.resolve("piano/topdown")
    assert np.array_equal(top.pos, [0, 0, 1.0])
    assert math.isclose(top.fovy, math.degrees(2 * math.atan2(0.5 * piano.BASE_SIZE[1], 1.0)), rel_tol=1e-15)
    assert np.allclose(top.rot, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)   # quat (1, 0, 0, 1): 90 degrees about z
    assert np.array_equal(cameras.resolve(5).rot, top.rot)
    # free camera (stage.py:27-30): looks at (0.2, 0, 0.3) from 1.5 * 0.6 away, azimuth 180, elevation -50
    free = cameras.resolve(-1)
    look = -free.rot[:, 2]
    assert np.allclose(free.pos + 0.9 * look, [0.2, 0, 0.3], atol=1e-15)
    assert np.allclose(look, [-math.cos(math.radians(50)), 0, -math.sin(math.radians(50))], atol=1e-15)
    assert np.allclose(free.rot[:, 0], [0, 1, 0], atol=1e-15) and free.fovy == 45.0
    custom = cameras.resolve(((1, 2, 3), np.eye(3), 60.0))
    assert np.array_equal(custom.pos, [1, 2, 3]) and custom.fovy == 60.0
    for bad in ("nosuch", "piano/nosuch", "hand/back"):
        with pytest.raises(ValueError):
            cameras.resolve(bad)
    for bad in (6, -2, ((0, 0, 0), np.eye(3), 0.0), (1, 2)):
        with pytest.raises(ValueError):
            cameras.resolve(bad)


# ---- closed forms through the host-compiled routine ------------------------------------------------------------------
BOX, CAPSULE, CYLINDER, SPHERE, MESH = range(5)   # csrc/rp_render.hpp: RPR_BOX ..
_BOX_CORNER_PLANES = np.array([[1, 0, 0, 0.1], [-1, 0, 0, 0.1], [0, 1, 0, 0.2], [0, -1, 0, 0.2], [0, 0, 1, 0.3], [0, 0, -1, 0.3]], float)


def _hit(gtype, size, o, d, **kw):
    t, n, rid = rr.trace_one(gtype, size, o, d, **kw)
    return t, n, rid


def test_closed_forms_box_and_hull():
    size = (0.1, 0.2, 0.3)
    hull = render_tables.hull_planes([[sx * 0.1, sy * 0.2, sz * 0.3] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    assert len(hull) == 6                                     # the 12 triangles of qhull merged into 6 faces
    for gtype, kw in ((BOX, {}), (MESH, dict(planes=hull))):
        for axis in range(3):
            for sign in (1.0, -1.0):
                o = np.zeros(3); o[axis] = 2.0 * sign; o[(axis + 1) % 3] = 0.05
                d = np.zeros(3); d[axis] = -sign
                t, n, rid = _hit(gtype, size, o, d, **kw)
                want = np.zeros(3); want[axis] = sign
                assert rid == 0 and abs(t - (2.0 - size[axis])) < 1e-6 and np.allclose(n, want, atol=1e-6)
                # unnormalised direction: t is the ray PARAMETER
                t2, _, _ = _hit(gtype, size, o, 2 * d, **kw)
                assert abs(t2 - 0.5 * (2.0 - size[axis])) < 1e-6
                # parallel miss: shifted beyond the face
                o2 = o.copy(); o2[(axis + 1) % 3] = size[(axis + 1) % 3] + 1e-3
                assert _hit(gtype, size, o2, d, **kw)[2] == -1
                # pointing away
                assert _hit(gtype, size, o, -d, **kw)[2] == -1
        # from inside: the exit, outward normal
        t, n, rid = _hit(gtype, size, (0.02, 0.0, 0.0), (1, 0, 0), **kw)
        assert rid == 0 and abs(t - 0.08) < 1e-6 and np.allclose(n, [1, 0, 0], atol=1e-6)
        # a diagonal ray at the face centre of +z
        t, n, rid = _hit(gtype, size, (0.05, 0.05, 1.3), (-0.05, -0.05, -1.0), **kw)
        assert rid == 0 and abs(t - 1.0) < 1e-6 and np.allclose(n, [0, 0, 1], atol=1e-6)


def test_closed_forms_capsule_cylinder_sphere():
    r, h = 0.05, 0.2
    # side of the cylinder part, along -x
    for gtype in (CAPSULE, CYLINDER):
        t, n, rid = _hit(gtype, (r, h), (1.0, 0, 0.1), (-1, 0, 0))
        assert rid == 0 and abs(t - 0.95) < 1e-6 and np.allclose(n, [1, 0, 0], atol=1e-6)
        t, n, rid = _hit(gtype, (r, h), (0, -1.0, -0.1), (0, 1, 0))
        assert rid == 0 and abs(t - 0.95) < 1e-6 and np.allclose(n, [0, -1, 0], atol=1e-6)
        assert _hit(gtype, (r, h), (1.0, r + 1e-3, 0), (-1, 0, 0))[2] == -1          # passes beside it
        assert _hit(gtype, (r, h), (r + 1e-3, 0, 1.0), (0, 0, -1))[2] == -1          # parallel to the axis, outside
        t, n, rid = _hit(gtype, (r, h), (0, 0, 0), (1, 0, 0))                        # from inside
        assert rid == 0 and abs(t - r) < 1e-6 and np.allclose(n, [1, 0, 0], atol=1e-6)
    # capsule cap: down the axis hits the pole; off axis hits the half sphere
    t, n, rid = _hit(CAPSULE, (r, h), (0, 0, 1.0), (0, 0, -1))
    assert rid == 0 and abs(t - (1.0 - h - r)) < 1e-6 and np.allclose(n, [0, 0, 1], atol=1e-6)
    x = 0.03
    t, n, rid = _hit(CAPSULE, (r, h), (x, 0, 1.0), (0, 0, -1))
    zc = math.sqrt(r * r - x * x)
    assert rid == 0 and abs(t - (1.0 - h - zc)) < 1e-6 and np.allclose(n, [x / r, 0, zc / r], atol=1e-5)
    t, n, rid = _hit(CAPSULE, (r, h), (1.0, 0, h + 0.03), (-1, 0, 0))                # side-on, above the cylinder part
    assert rid == 0 and abs(t - (1.0 - 0.04)) < 1e-6 and np.allclose(n, [0.8, 0, 0.6], atol=1e-5)
    assert _hit(CAPSULE, (r, h), (1.0, 0, h + r + 1e-3), (-1, 0, 0))[2] == -1
    t, n, rid = _hit(CAPSULE, (r, h), (0, 0, 0), (0, 0, 1))                          # from inside along the axis
    assert rid == 0 and abs(t - (h + r)) < 1e-6 and np.allclose(n, [0, 0, 1], atol=1e-6)
    # cylinder cap: flat
    t, n, rid = _hit(CYLINDER, (r, h), (x, 0, 1.0), (0, 0, -1))
    assert rid == 0 and abs(t - (1.0 - h)) < 1e-6 and np.allclose(n, [0, 0, 1], atol=1e-6)
    t, n, rid = _hit(CYLINDER, (r, h), (x, 0, -1.0), (0, 0, 1))
    assert rid == 0 and abs(t - (1.0 - h)) < 1e-6 and np.allclose(n, [0, 0, -1], atol=1e-6)
    assert _hit(CYLINDER, (r, h), (1.0, 0, h + 1e-3), (-1, 0, 0))[2] == -1           # parallel to the cap, above it
    t, n, rid = _hit(CYLINDER, (r, h), (0.02, 0, 0), (0, 0, 1))                      # from inside through the cap
    assert rid == 0 and abs(t - h) < 1e-6 and np.allclose(n, [0, 0, 1], atol=1e-6)
    # sphere
    t, n, rid = _hit(SPHERE, (r,), (0, 0.03, 1.0), (0, 0, -1))
    assert rid == 0 and abs(t - (1.0 - 0.04)) < 1e-6 and np.allclose(n, [0, 0.6, 0.8], atol=1e-5)
    assert _hit(SPHERE, (r,), (0, r + 1e-3, 1.0), (0, 0, -1))[2] == -1
    t, n, rid = _hit(SPHERE, (r,), (0, 0, 0), (0, 1, 0))
    assert rid == 0 and abs(t - r) < 1e-6 and np.allclose(n, [0, 1, 0], atol=1e-6)


def test_closed_forms_floor_and_ties():
    # the floor square's edge: |x|, |y| <= 1 at z = 0
    for x, want in ((0.999, 1), (1.001, -1)):
        t, n, rid = rr.trace_one(-1, (0, 0, 0), (x, 0.5, 2.0), (0, 0, -1), floor_half=1.0)
        assert rid == want
        if want == 1:
            assert abs(t - 2.0) < 1e-6 and np.allclose(n, [0, 0, 1])
    assert rr.trace_one(-1, (0, 0, 0), (0, 0, 2.0), (1, 0, 0), floor_half=1.0)[2] == -1       # parallel to the floor
    assert rr.trace_one(-1, (0, 0, 0), (0, 0, 2.0), (0, 0, 1), floor_half=1.0)[2] == -1       # looking up
    # a hull whose bottom face lies IN the floor plane, seen from below: an exact tie -> the lower id (the hull)
    slab = np.array([[1, 0, 0, 0.5], [-1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, -1, 0, 0.5], [0, 0, 1, 0.5], [0, 0, -1, 0.0]], float)
    t, n, rid = rr.trace_one(MESH, (0.5, 0.5, 0.5), (0, 0, -2.0), (0, 0, 1), planes=slab, floor_half=1.0)
    assert rid == 0 and t == 2.0 and np.allclose(n, [0, 0, -1])
    assert rr.trace_one(-1, (0, 0, 0), (0, 0, -2.0), (0, 0, 1), floor_half=1.0)[0] == 2.0     # (the floor alone: the same t)
    # the box in front of the floor
    t, n, rid = rr.trace_one(BOX, (0.1, 0.1, 0.1), (0, 0, 2.0), (0, 0, -1), floor_half=1.0)
    assert rid == 0 and abs(t - 1.9) < 1e-6
    t, n, rid = rr.trace_one(BOX, (0.1, 0.1, 0.1), (0.5, 0, 2.0), (0, 0, -1), floor_half=1.0)
    assert rid == 1 and abs(t - 2.0) < 1e-6


# ---- whole images ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_renderers():
    return {name: rr.HostRenderer(rr.build_scene_variant(name), 1) for name in rr.SCENES}


def test_reference_rounding_supports_the_tolerance():
    """The float32 evaluation of the reference against its float64 evaluation: the depth tolerance is 4 x the largest
    difference, and the reference alone stays under a quarter of the segmentation cap on every camera."""
    worst_d, worst_s = rr.measure_reference_rounding()
    print(f"reference rounding: depth {worst_d:.4e}, segmentation per camera {worst_s}")
    assert worst_d <= rr.MEASURED_DEPTH_ROUNDING * 1.0005, "the recorded measurement no longer holds: re-measure"
    assert rr.DEPTH_TOL == 4 * rr.MEASURED_DEPTH_ROUNDING
    for cam, frac in worst_s.items():
        assert frac < rr.SEG_CAP / 4, f"camera {cam}: the reference's own disagreement {frac:.4f} is not under a quarter of the cap"


@pytest.mark.parametrize("cam", rr.CAMERAS, ids=str)
@pytest.mark.parametrize("case", range(len(rr.SCENES)), ids=rr.SCENES)
def test_host_images_match_the_reference(host_renderers, case, cam):
    name, pose, q = rr.image_cases()[case]
    got = host_renderers[name].render(q, cam)
    ref = rr.reference_for(name, q, cam)
    assert len(np.unique(ref[2])) > 5, "the case shows too little to test anything"
    rr.compare_images((got[0][0], got[1][0], got[2][0]), ref, label=f"host {name}/{pose}/{cam}")


def test_host_geom_frames_match_the_oracle(host_renderers):
    for name, _, q in rr.image_cases():
        for prec in (64, 32):
            hr = rr.HostRenderer(rr.build_scene_variant(name), 1, precision=prec)
            hr.render(q, "back")
            xp, xm = hr.geom_frames()
            op, om = rr.oracle_geom_poses(rr.build_scene_variant(name), q)
            tol = 1e-6
            assert np.abs(xp[0] - op).max() < tol and np.abs(xm[0] - om).max() < tol


def test_host_tree_offset_key_rgb_and_refusals():
    si = rr.build_scene_variant("capsule")
    m = si.model
    hr = rr.HostRenderer(si, 2, colorize_fingertips=True)
    q = rr.image_cases()[0][2]
    off = np.zeros((2, 2, 3)); off[1, 0] = (0.01, -0.03, 0.02)
    krgb = np.zeros((2, 88, 3), np.uint8)
    krgb[:] = np.where(np.array([piano.is_key_black(k) for k in range(88)])[None, :, None], 26, 230)
    root = int(render_tables.hand_root_bodies(m, si.key_joint_ids)[0])
    op, om = rr.oracle_geom_poses(si, q, {root: off[1, 0]})
    seg0 = rr.reference_render(si, op, om, "back")[2]
    red = int(np.argmax([(seg0 == g).sum() for g in si.key_geom_ids]))      # the key that shows most pixels
    krgb[1, red] = (255, 0, 0)
    out = hr.render(q, "back", tree_offset=off, key_rgb=krgb)
    xp, xm = hr.geom_frames()
    assert np.abs(xp[1] - op).max() < 1e-6 and np.abs(xm[1] - om).max() < 1e-6
    assert np.abs(xp[0] - op).max() > 1e-3       # env 0 carries no offset
    ref = rr.reference_render(si, op, om, "back", key_rgb=krgb[1], colorize_fingertips=True)
    rr.compare_images((out[0][1], out[1][1], out[2][1]), ref, label="host offset + key_rgb + fingertip colours")
    assert (ref[2] == si.key_geom_ids[red]).sum() > 0
    assert (ref[0][ref[2] == si.key_geom_ids[red]] == (255, 0, 0))[:, 1:].all()   # (red key: green and blue stay 0)
    assert (out[0][1][out[2][1] == si.key_geom_ids[red]][:, 0] > 90).all()
    # env range: only env 1 is written
    buf = (np.full((2, rr.H, rr.W, 3), 7, np.uint8), np.full((2, rr.H, rr.W), -3.0, np.float32), np.full((2, rr.H, rr.W), -9, np.int32))
    hr.render(q, "back", tree_offset=off, key_rgb=krgb, env_first=1, env_count=1, out=buf)
    assert (buf[0][0] == 7).all() and (buf[1][0] == -3.0).all() and (buf[2][0] == -9).all()
    assert np.array_equal(buf[2][1], out[2][1]) and np.array_equal(buf[0][1], out[0][1])
    # refusals, with a message
    for kw, word in ((dict(height=0), "image size"), (dict(env_first=1, env_count=2), "outside the batch"),
                     (dict(env_first=-1), "outside the batch"), (dict(env_count=0), "outside the batch")):
        with pytest.raises(RuntimeError, match=word):
            hr.render(q, "back", **kw)


# ---- the key-colour rule ---------------------------------------------------------------------------------------------
def _bound_task(**task_kwargs):
    from robopianist_amd import music
    from robopianist_amd.suite.tasks import piano_with_shadow_hands as task_lib
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        task = task_lib.PianoWithShadowHands(midi=music.load("TwinkleTwinkleRousseau"), primitive_fingertip_collisions=True,
                                             **task_kwargs)
    phys = FakePhysics(task.scene, 3)
    task.bind(phys, 3, np.random.RandomState(0))
    return task, phys


def test_key_rgb_rule():
    white, black, green = (230, 230, 230), (26, 26, 26), (51, 204, 51)
    tips = [(204, 51, 204), (204, 51, 51), (51, 204, 204), (51, 51, 204), (204, 204, 51)]
    task, phys = _bound_task(change_color_on_activation=True)
    assert task.colorize_fingertips
    # hand-made state: env 0 nothing; env 1: key 39 (white) in the fingering set with finger 1 (right index), pressed
    # key 40 (black) not in the set; env 2: key 39 in the set AND pressed, key 44 in the set with the left hand's
    # finger 7 (-> colour 2), key 46 in the set without fingering (-> little finger)
    task._goal_current.zero_(); task._finger_current.fill_(-1); task.piano._activation.zero_()
    task._goal_current[1, 39] = 1; task._finger_current[1, 39] = 1; task.piano._activation[1, 40] = True
    task._goal_current[2, 39] = 1; task._finger_current[2, 39] = 1; task.piano._activation[2, 39] = True
    task._goal_current[2, 44] = 1; task._finger_current[2, 44] = 7
    task._goal_current[2, 46] = 1
    want = np.zeros((3, 88, 3), np.uint8)
    for k in range(88):
        want[:, k] = black if piano.is_key_black(k) else white
    assert piano.is_key_black(40) and not piano.is_key_black(39)
    want[1, 39] = tips[1]; want[1, 40] = green
    want[2, 39] = green; want[2, 44] = tips[2]; want[2, 46] = tips[4]
    got = task.key_rgb(phys)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 88, 3) and got.is_contiguous()
    assert np.array_equal(got.numpy(), want)
    # change_color_on_activation off: pressed keys keep their base colour, the fingering colours stay
    task2, phys2 = _bound_task(change_color_on_activation=False)
    for name in ("_goal_current", "_finger_current"):
        getattr(task2, name).copy_(getattr(task, name))
    task2.piano._activation.copy_(task.piano._activation)
    want2 = want.copy(); want2[1, 40] = black; want2[2, 39] = white
    assert np.array_equal(task2.key_rgb(phys2).numpy(), want2)
    # colourisation off (either switch): only the activation colour is left
    for kw in (dict(disable_colorization=True), dict(disable_fingering_reward=True)):
        task3, phys3 = _bound_task(change_color_on_activation=True, **kw)
        assert not task3.colorize_fingertips
        for name in ("_goal_current", "_finger_current"):
            getattr(task3, name).copy_(getattr(task, name))
        task3.piano._activation.copy_(task.piano._activation)
        want3 = want.copy(); want3[1, 39] = white; want3[2, 44] = white; want3[2, 46] = black if piano.is_key_black(46) else white
        assert np.array_equal(task3.key_rgb(phys3).numpy(), want3)


# ---- the binding ---------------------------------------------------------------------------------------------------
def test_render_abi_struct_and_symbols_match_the_header():
    """The ctypes mirror lists rp_render_args' fields in the header's order, and the binding names every entry point the
    header declares (the header lives in include/render/: librp_render.so is not librp_engine.so)."""
    import os
    import re
    from robopianist_amd import render
    src = open(os.path.join(rr.ROOT, "include", "render", "rp_render.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct rp_render_args \{(.*?)\} rp_render_args;", src, flags=re.S).group(1)
    names = []
    for stmt in body.split(";"):
        for part in stmt.strip().split(",") if stmt.strip() else []:
            names.append(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", re.sub(r"\[\d+\]", "", part))[-1])
    assert names == [f[0] for f in render.RenderArgs._fields_]
    assert names[0] == "struct_size"
    assert sorted(set(re.findall(r"\b(rp_render[a-z_0-9]*)\s*\(", src))) == sorted(render.EXPORTED_SYMBOLS)
    with pytest.raises(render.RenderError, match="not found"):
        render.load_library(os.path.join(rr.ROOT, "no_such_dir", "librp_render.so"))


def test_closed_forms_grazing_the_bounding_sphere():
    """Rays that touch a shape where it touches its bounding sphere, with the radius the tables give the kernel's
    float32 reject (render_tables.bounding_radius): the reject must let them through to the exact test."""
    # a sphere IS its bounding sphere: a ray a micrometre inside the silhouette hits, one outside the slack misses
    r = 0.0075
    rb = float(render_tables.bounding_radius(r))
    t, n, rid = rr.trace_one(SPHERE, (r,), (r - 1e-6, 0, 1.0), (0, 0, -1), rbound=rb)
    # (the chord is 2 x 1.22e-4 long and float32 cannot place its ends from a metre away: the hit lies on it)
    assert rid == 0 and abs(t - 1.0) <= 1.01 * math.sqrt(r * r - (r - 1e-6) ** 2) + 1e-6
    assert rr.trace_one(SPHERE, (r,), (rb + 1e-5, 0, 1.0), (0, 0, -1), rbound=rb)[2] == -1
    # the same from a camera's distance and off the axes, where the reject's b^2 - a c cancels most
    o = np.array([0.6, -0.4, 0.9]); c = np.array([0.0, 0.0, 0.0])
    u = np.cross(o - c, [0, 0, 1.0]); u /= np.linalg.norm(u)
    for inside, want in ((r - 2e-6, 0), (rb + 2e-5, -1)):
        target = c + inside * u                      # closest approach of the ray to the centre
        assert rr.trace_one(SPHERE, (r,), o, target - o, rbound=rb)[2] == want
    # a box touches its bounding sphere at its corners: a ray tangent to the sphere through a point just inside a corner
    size = np.array([0.1, 0.2, 0.3])
    rb = float(render_tables.bounding_radius(np.linalg.norm(size)))
    p = size * (1 - 1e-5)
    d = np.array([0.2, -0.1, 0.0]) / math.hypot(0.2, 0.1)        # perpendicular to the corner's direction
    t, n, rid = rr.trace_one(BOX, size, p - d, d, rbound=rb)
    assert rid == 0 and 0.99 < t < 1.0
    # a capsule touches it at its poles
    rad, h = 0.0075, 0.0065
    rb = float(render_tables.bounding_radius(rad + h))
    t, n, rid = rr.trace_one(CAPSULE, (rad, h), (-1.0, 0, (rad + h) * (1 - 1e-5)), (1, 0, 0), rbound=rb)
    assert rid == 0 and abs(t - 1.0) < 1e-3 and n[2] > 0.99


def test_launch_slices_cover_a_large_batch_once():
    """rp_render cuts a call of more than 65535 envs (the grid's y limit) into slices: every env in exactly one slice,
    no slice larger than the limit.  (tests/test_gpu_render.py renders 65540 envs in one call; the arithmetic is checked here.)"""
    L = rr.host_library()
    for n in (1, 5, 65535, 65536, 131070, 131071, 200000):
        buf = np.zeros((8, 2), np.int32)
        k = L.rph_slices(n, buf.ctypes.data, 8)
        firsts, counts = buf[:k, 0], buf[:k, 1]
        assert k == -(-n // 65535) and (counts > 0).all() and counts.max() <= 65535
        assert firsts[0] == 0 and np.array_equal(firsts[1:], np.cumsum(counts)[:-1]) and counts.sum() == n


# ---- the wide cases (tests/render_reference.py: wide_cases) --------------------------------------------------------
def test_wide_cases_stay_inside_the_recorded_rounding():
    """The reference in float32 against itself in float64 on every wide case and on the mixed batch: the depth rounding
    stays under the figure the tolerance was derived from and the segmentation disagreement under a quarter of the cap,
    so the cases are judged by the bounds on record.  Every case shows what it is there for."""
    ids, cases = rr.wide_case_ids(), rr.wide_cases()
    assert len(ids) == len(cases) == 32 and len(set(ids)) == 32
    worst_d = worst_s = 0.0
    for cid, (name, q, off, cam, h, w, krgb, tips) in zip(ids, cases):
        kw = dict(offsets=off, height=h, width=w)
        r64 = rr.reference_for(name, q, cam, np.float64, **kw); r32 = rr.reference_for(name, q, cam, np.float32, **kw)
        dd, frac = rr.reference_rounding(r64, r32)
        shown = len(np.unique(r64[2]))
        print(f"reference f32 vs f64: {cid:28s} depth {dd:.4e} seg {100 * frac:.4f} % ids shown {shown}")
        worst_d, worst_s = max(worst_d, dd), max(worst_s, frac)
        assert dd <= rr.MEASURED_DEPTH_ROUNDING, f"{cid}: depth rounding {dd:.4e}: choose another size or pose"
        assert frac < rr.SEG_CAP / 4, f"{cid}: the reference's own disagreement {frac:.4f}: choose another size or pose"
        if cid.startswith("away"):
            assert (r64[2] == -1).all() and np.isposinf(r64[1]).all()
            assert (r64[0] == r64[0][0, 0]).all()
        elif (h, w) not in ((1, 1), (3, 171)) and not cid.startswith("inside_base"):   # (inside a shape: that shape alone)
            assert shown > 5, f"{cid}: the case shows too little to test anything"
        if cid.startswith("down"):
            # the centre row and the centre column: a ray component that is exactly 0, in float32 as the kernel casts them
            _, d = rr.pixel_rays(cam, h, w, np.float32)
            zero = (d == 0).any(1).reshape(h, w)
            assert zero[h // 2].all() and zero[:, w // 2].all() and zero.sum() == h + w - 1
            # the keys' and the base's frames are axis-aligned at the zero pose, so those rays keep their exact zero in the
            # geom frame: the ones through the base take the box's parallel-slab branch and hit, the same rays miss the
            # keys to either side of them through it
            si = rr.build_scene_variant(name)
            xmat = rr.oracle_geom_poses(si, q)[1]
            assert all(np.isin(xmat[g], (0.0, 1.0, -1.0)).all() for g in si.key_geom_ids)
            aligned = [g for g in np.unique(r64[2][zero]) if 0 <= g < si.model.ngeom and np.isin(xmat[g], (0.0, 1.0, -1.0)).all()]
            print(f"  {cid}: {int(zero.sum())} rays with an exactly zero component, axis-aligned geoms under them: {aligned}")
            assert len(aligned) >= 1, f"{cid}: no axis-aligned geom under the zero-component rays"
        if cid.startswith("inside_base"):
            # every pixel is resolved through the exit branch, and shows the base from inside: two of its faces
            n_exit = rr.reference_stats_for(name, q, cam, np.float64, **kw)["exit_pixels"]
            print(f"  {cid}: {n_exit} pixels resolved through the exit branch, {len(np.unique(r64[0][..., 0]))} shades")
            assert n_exit == h * w and (r64[2] == 0).all()
            assert rr.build_scene_variant(name).model.names["geom"][0] == "piano/base_geom"
            assert r64[1].max() < 0.11 and len(np.unique(r64[0][..., 0])) >= 2
        if cid.startswith("far_corner"):
            m = rr.build_scene_variant(name).model
            assert (r64[2] == m.ngeom).any() and (r64[2] == -1).any() and r64[1][np.isfinite(r64[1])].max() > 3.5
        if cid.startswith("below"):
            assert (r64[2] == rr.build_scene_variant(name).model.ngeom).any()
        if krgb is not None:
            si = rr.build_scene_variant(name)
            key = int(np.flatnonzero((krgb == rr.MAGENTA).all(1))[0])
            ref = rr.reference_for(name, q, cam, np.float64, key_rgb=krgb, colorize_fingertips=tips, **kw)
            on_key = ref[2] == si.key_geom_ids[key]
            assert on_key.sum() > 0 and (ref[0][on_key][:, 1] == 0).all() and (ref[0][on_key][:, 0] > 90).all()
    q, off, krgb = rr.mixed_batch()
    for e in range(rr.MIXED_ENVS):
        kw = dict(offsets=off[e], key_rgb=krgb[e], colorize_fingertips=True)
        dd, frac = rr.reference_rounding(rr.reference_for("capsule", q[e], "back", np.float64, **kw),
                                         rr.reference_for("capsule", q[e], "back", np.float32, **kw))
        print(f"reference f32 vs f64: mixed batch env {e}            depth {dd:.4e} seg {100 * frac:.4f} %")
        worst_d, worst_s = max(worst_d, dd), max(worst_s, frac)
        assert dd <= rr.MEASURED_DEPTH_ROUNDING and frac < rr.SEG_CAP / 4
    print(f"wide cases: worst depth rounding {worst_d:.4e} (on record {rr.MEASURED_DEPTH_ROUNDING:.4e}), "
          f"worst segmentation disagreement {100 * worst_s:.4f} % (cap / 4 = {100 * rr.SEG_CAP / 4:.2f} %)")


@pytest.fixture(scope="module")
def wide_host_renderers():
    return {(name, tips): rr.HostRenderer(rr.build_scene_variant(name), 1, colorize_fingertips=tips)
            for name, tips in {(c[0], c[7]) for c in rr.wide_cases()}}


@pytest.mark.parametrize("case", range(len(rr.wide_case_ids())), ids=rr.wide_case_ids())
def test_host_wide_cases_match_the_reference(wide_host_renderers, case):
    """csrc/rp_render.hpp on the CPU over the wide cases: a bug in the shared per-ray code shows here without a GPU."""
    name, q, off, cam, h, w, krgb, tips = rr.wide_cases()[case]
    got = wide_host_renderers[(name, tips)].render(q, cam, h, w, tree_offset=None if off is None else off[None],
                                                   key_rgb=None if krgb is None else krgb[None])
    ref = rr.reference_for(name, q, cam, offsets=off, height=h, width=w,
                           **(dict(key_rgb=krgb, colorize_fingertips=tips) if krgb is not None else {}))
    rr.compare_images((got[0][0], got[1][0], got[2][0]), ref, label=f"host {rr.wide_case_ids()[case]}")


def test_host_mixed_batch_matches_the_reference():
    """Five envs, each with its own pose, tree offsets and key colours, against the reference of each."""
    q, off, krgb = rr.mixed_batch()
    hr = rr.HostRenderer(rr.build_scene_variant("capsule"), rr.MIXED_ENVS, colorize_fingertips=True)
    out = hr.render(q, "back", tree_offset=off, key_rgb=krgb)
    for e in range(rr.MIXED_ENVS):
        ref = rr.reference_for("capsule", q[e], "back", offsets=off[e], key_rgb=krgb[e], colorize_fingertips=True)
        rr.compare_images((out[0][e], out[1][e], out[2][e]), ref, label=f"host mixed batch env {e}")
    assert not np.array_equal(out[2][0], out[2][1])


def test_closed_forms_capsule_seam():
    """Rays aimed AT the seam circle of a capsule, where its cylinder meets a half sphere: both parts describe that point,
    and rounding must not leave the root to neither (RPR_CAP_EPS; without it one such ray in nine falls through to the
    far side or misses).  2000 rays from 0.3 .. 1 m at a finger-sized capsule, incidence cosine >= 0.5, against the
    reference's exact span of the same float32 ray.  Tolerance 1e-4 in the ray parameter (t is about 1): the float32
    cancellation in b^2 - a c moves a root by about eps L / (r cos) = 1.2e-7 x 1 / (0.009 x 0.5) = 2.6e-5; 4 x that."""
    r, hh = 0.009, 0.02
    rng = np.random.default_rng(5)
    n_rays = 2000
    phi = rng.uniform(0, 2 * np.pi, n_rays)
    radial = np.stack([np.cos(phi), np.sin(phi), np.zeros(n_rays)], 1)
    seam = r * radial + np.array([0, 0, hh])[None, :] * rng.choice([-1.0, 1.0], n_rays)[:, None]
    side = rng.normal(size=(n_rays, 3))
    side -= radial * (side * radial).sum(1)[:, None]
    side /= np.linalg.norm(side, axis=1)[:, None]
    cosi = rng.uniform(0.5, 1.0, n_rays)
    back = cosi[:, None] * radial + np.sqrt(1 - cosi ** 2)[:, None] * side          # from the seam point to the origin
    o = (seam + back * rng.uniform(0.3, 1.0, n_rays)[:, None]).astype(np.float32)
    d = (seam - o.astype(np.float64)).astype(np.float32)
    t0, _, n0, _, hit = rr.shape_span(spec.GEOM_CAPSULE, np.array([r, hh, 0.0]), None, o.astype(np.float64), d.astype(np.float64), np.float64)
    assert hit.sum() > 0.9 * n_rays
    worst_t = worst_n = 0.0
    for i in np.flatnonzero(hit):
        t, n, rid = rr.trace_one(CAPSULE, (r, hh), o[i], d[i])
        assert rid == 0, f"ray {i} at the seam misses the capsule"
        worst_t = max(worst_t, abs(t - t0[i])); worst_n = max(worst_n, np.abs(n - n0[i]).max())
    print(f"capsule seam: max |t - exact| {worst_t:.3e}, max normal difference {worst_n:.3e}")
    assert worst_t <= 1e-4
    assert worst_n <= 1e-4 / r * 2      # (a point moved by 1e-4 x 1 m along the ray turns the normal by that over r)
