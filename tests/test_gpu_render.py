"""GPU tests of the camera renderer (include/render/rp_render.h, librp_render.so) and the pixel observation wrapper.

Images are 30 x 44 (H W = 1320 is no multiple of 256: the last workgroup of every image is partial), E <= 5.  The
numpy reference, the cases, the 1 % segmentation cap and the depth tolerance are the CPU suite's
(tests/render_reference.py: the reference in float32 against itself in float64 differs by 5.4969e-05 in depth on these
images; DEPTH_TOL = 4 x that = 2.1988e-04).

The second half of the file widens that: the wide cases of tests/render_reference.py (image ends on and next to a
workgroup boundary, rays with exactly zero components, cameras below, inside, far from and facing away from the scene,
tree offsets and key colours) at precision 64 and 32 under the same cap and tolerance, one batch whose envs all differ,
guard bytes around caller-owned outputs, 65540 envs in one call, and a render on a stream of its own.
"""
import os
import warnings

import numpy as np
import pytest
import torch

import render_reference as rr
from robopianist_amd.model import piano, render_tables

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(x):
    return x.detach().cpu().numpy()


def _physics(name, n_envs, precision=64):
    from robopianist_amd.suite.physics import TorchPhysics
    return TorchPhysics(rr.build_scene_variant(name), n_envs, precision=precision)


def _set_qpos(phys, q):
    phys.qpos.copy_(torch.as_tensor(np.asarray(q), device=phys.device, dtype=phys.dtype))


@pytest.mark.parametrize("precision", (64, 32))
def test_geom_frames_match_the_oracle(precision):
    """Reset pose, two random poses and one with a non-zero RP_TREE_OFFSET on the right hand (the oracle sees the offset
    as the root body's body_pos).  1e-6 absolute: the kinematics run in T and are stored as float, four float ulps at
    2 m are 9.5e-7."""
    si = rr.build_scene_variant("capsule")
    m = si.model
    phys = _physics("capsule", 4, precision)
    poses = [np.zeros(m.nv), rr.random_pose(m, 1), rr.random_pose(m, 2), rr.random_pose(m, 3)]
    off = np.zeros((4, 2, 3)); off[3, 0] = (0.0, 0.02, -0.05)
    _set_qpos(phys, np.stack(poses))
    phys.set_tree_offset(off)
    phys.render(rr.H, rr.W, "back")
    xp, xm = phys.renderer().geom_frames()
    root = int(render_tables.hand_root_bodies(m, si.key_joint_ids)[0])
    worst = 0.0
    for e, q in enumerate(poses):
        # (the fp32 engine holds qpos in float: the oracle gets the same rounded angles)
        qe = q.astype(np.float32).astype(np.float64) if precision == 32 else q
        offs = {root: off[e, 0].astype(np.float32).astype(np.float64) if precision == 32 else off[e, 0]} if e == 3 else None
        op, om = rr.oracle_geom_poses(si, qe, offs)
        worst = max(worst, np.abs(xp[e] - op).max(), np.abs(xm[e] - om).max())
    print(f"geom frames vs oracle, precision {precision}: max abs err {worst:.3e}")
    assert worst < 1e-6
    assert np.abs(xp[3] - xp[2]).max() > 1e-2


@pytest.mark.parametrize("case", range(len(rr.SCENES)), ids=rr.SCENES)
def test_images_match_the_reference(case):
    name, pose, q = rr.image_cases()[case]
    phys = _physics(name, 2)
    _set_qpos(phys, np.stack([q, q]))
    for cam in rr.CAMERAS:
        rgb = _np(phys.render(rr.H, rr.W, cam))[1].copy()
        depth = _np(phys.render(rr.H, rr.W, cam, depth=True))[1].copy()
        seg = _np(phys.render(rr.H, rr.W, cam, segmentation=True))[1].copy()
        assert rgb.dtype == np.uint8 and depth.dtype == np.float32 and seg.dtype == np.int32
        rr.compare_images((rgb, depth, seg), rr.reference_for(name, q, cam), label=f"gpu {name}/{pose}/{cam}")


def test_env_indexing_and_env_range():
    si = rr.build_scene_variant("capsule")
    m = si.model
    poses = np.stack([rr.random_pose(m, 20 + i) for i in range(5)])
    phys5 = _physics("capsule", 5)
    _set_qpos(phys5, poses)
    r5 = phys5.renderer()
    out5 = [x.clone() for x in r5.render(phys5.qpos, rr.H, rr.W, "closeup", rgb=True, depth=True, segmentation=True)]
    phys1 = _physics("capsule", 1)
    for e in range(5):
        _set_qpos(phys1, poses[e:e + 1])
        out1 = phys1.renderer().render(phys1.qpos, rr.H, rr.W, "closeup", rgb=True, depth=True, segmentation=True)
        for a, b in zip(out5, out1):
            assert torch.equal(a[e], b[0]), f"env {e} of the batch differs from the 1-env render of its pose"
    assert not torch.equal(out5[2][0], out5[2][1])
    # env_first = 2, env_count = 2 writes exactly those two images
    bufs = r5.outputs(rr.H, rr.W)
    bufs[0].fill_(7); bufs[1].fill_(-3.0); bufs[2].fill_(-9)
    r5.render(phys5.qpos, rr.H, rr.W, "closeup", rgb=True, depth=True, segmentation=True, env_first=2, env_count=2)
    torch.cuda.synchronize()
    for e in range(5):
        if e in (2, 3):
            assert all(torch.equal(b[e], o[e]) for b, o in zip(bufs, out5))
        else:
            assert bool((bufs[0][e] == 7).all()) and bool((bufs[1][e] == -3.0).all()) and bool((bufs[2][e] == -9).all())


def test_key_rgb_changes_exactly_that_keys_pixels():
    si = rr.build_scene_variant("capsule")
    phys = _physics("capsule", 3)
    _set_qpos(phys, np.zeros((3, si.model.nv)))
    base = np.zeros((3, 88, 3), np.uint8)
    base[:] = np.where(np.array([piano.is_key_black(k) for k in range(88)])[None, :, None], 26, 230)
    seg = _np(phys.render(rr.H, rr.W, "topdown", segmentation=True)).copy()
    key = int(np.argmax([(seg[1] == g).sum() for g in si.key_geom_ids]))
    assert (seg[1] == si.key_geom_ids[key]).sum() > 0
    before = _np(phys.render(rr.H, rr.W, "topdown", key_rgb=torch.as_tensor(base))).copy()
    coloured = base.copy(); coloured[1, key] = (255, 0, 255)
    after = _np(phys.render(rr.H, rr.W, "topdown", key_rgb=torch.as_tensor(coloured))).copy()
    changed = (before != after).any(-1)
    assert not changed[0].any() and not changed[2].any()
    assert np.array_equal(changed[1], seg[1] == si.key_geom_ids[key])
    # without key_rgb the keys carry their base colours (0.9 / 0.1, within a level of the uint8 table)
    plain = _np(phys.render(rr.H, rr.W, "topdown")).copy()
    assert np.abs(plain.astype(int) - before.astype(int)).max() <= 1


def test_render_follows_step_in_stream_order():
    """render() straight after step(), no synchronisation in between, equals the render after rp_sync."""
    from robopianist_amd import suite
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", n_envs=4, seed=3,
                         task_kwargs=dict(primitive_fingertip_collisions=True, gravity_compensation=True))
    env.reset()
    spec = env.action_spec()
    rng = np.random.RandomState(0)
    for _ in range(3):
        env.step(rng.uniform(spec.minimum, spec.maximum, size=(4,) + spec.shape))
    env.step(rng.uniform(spec.minimum, spec.maximum, size=(4,) + spec.shape))
    a = env.physics.render(rr.H, rr.W, "back").clone()        # enqueued behind the step's kernels
    env.physics.engine.sync()
    torch.cuda.synchronize()
    b = env.physics.render(rr.H, rr.W, "back").clone()
    assert torch.equal(a, b)
    assert len(torch.unique(a)) > 3


def test_pixel_wrapper():
    from robopianist_amd import suite
    from robopianist_amd.wrappers import CanonicalSpecWrapper, PixelWrapper

    def load():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            env = suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", n_envs=4,
                             task_kwargs=dict(trim_silence=True, gravity_compensation=True, primitive_fingertip_collisions=True,
                                              n_steps_lookahead=10, change_color_on_activation=True))
        return CanonicalSpecWrapper(env)
    plain = load()
    wrapped = PixelWrapper(load(), render_kwargs=dict(height=rr.H, width=rr.W, camera_id="piano/back"))
    spec = wrapped.observation_spec()
    assert spec["pixels"].shape == (rr.H, rr.W, 3) and spec["pixels"].dtype == np.uint8
    assert set(spec) == set(plain.observation_spec()) | {"pixels"}
    assert wrapped.physics is wrapped._environment.physics            # __getattr__ passes through
    actions = np.load(os.path.join(ROOT, "tests", "golden", "twinkle_twinkle_actions.npy"))
    tp, tw = plain.reset(), wrapped.reset()
    assert "pixels" in tw.observation and "pixels" not in tp.observation
    first = tw.observation["pixels"].clone()
    assert tuple(first.shape) == (4, rr.H, rr.W, 3) and first.dtype == torch.uint8 and first.is_cuda
    for t in range(20):
        a = np.tile(actions[t], (4, 1))
        tp, tw = plain.step(a), wrapped.step(a)
        assert "pixels" in tw.observation
        assert torch.equal(tp.reward, tw.reward)
    assert torch.equal(plain.physics.qpos, wrapped.physics.qpos) and torch.equal(plain.physics.qvel, wrapped.physics.qvel)
    for k in tp.observation:
        assert torch.equal(tp.observation[k], tw.observation[k])
    assert not torch.equal(first, tw.observation["pixels"]), "the image did not change in 20 steps of the replay"
    # depth through the wrapper
    d = PixelWrapper(wrapped._environment, render_kwargs=dict(height=rr.H, width=rr.W, camera_id=3, depth=True),
                     observation_key="depth")
    assert d.observation_spec()["depth"].shape == (rr.H, rr.W) and d.observation_spec()["depth"].dtype == np.float32


def test_refusals_launch_nothing():
    from robopianist_amd import render
    si = rr.build_scene_variant("capsule")
    phys = _physics("capsule", 2)
    r = phys.renderer()
    bufs = r.outputs(rr.H, rr.W)
    bufs[0].fill_(7); bufs[1].fill_(-3.0); bufs[2].fill_(-9)
    torch.cuda.synchronize()

    def args(**kw):
        d = dict(camera="back", height=rr.H, width=rr.W, env_first=0, env_count=2, qpos=phys.qpos.data_ptr(),
                 rgb=bufs[0].data_ptr(), depth=bufs[1].data_ptr(), segmentation=bufs[2].data_ptr(),
                 hip_stream=torch.cuda.current_stream().cuda_stream)
        d.update(kw)
        return render.make_args(d.pop("camera"), d.pop("height"), d.pop("width"), d.pop("env_first"), d.pop("env_count"), **d)
    for a, word in ((args(height=0), "image size"), (args(qpos=None), "qpos is NULL"),
                    (args(env_first=1, env_count=2), "outside the batch")):
        assert r.render_raw(a) != 0
        assert word in r.last_error(), r.last_error()
    bad = args(); bad.struct_size = bad.struct_size - 8
    assert r.render_raw(bad) != 0 and "struct_size" in r.last_error()
    torch.cuda.synchronize()
    assert bool((bufs[0] == 7).all()) and bool((bufs[1] == -3.0).all()) and bool((bufs[2] == -9).all())
    assert r.render_raw(args()) == 0
    torch.cuda.synchronize()
    assert not bool((bufs[2] == -9).any())
    with pytest.raises(render.RenderError):
        phys.render(0, rr.W)


def test_renderer_is_lazy():
    """An env that never renders holds no renderer."""
    phys = _physics("capsule", 1)
    assert "_renderers" not in phys.__dict__
    phys.render(rr.H, rr.W)
    assert len(phys.__dict__["_renderers"]) == 1


# ---- the wide cases (tests/render_reference.py: wide_cases; tests/test_render_host.py runs them on the CPU first) ----
_bare = {}


def _renderer(name, n_envs, precision=64, colorize_fingertips=False):
    """A renderer without an engine (robopianist_amd/render.py), one per process and configuration."""
    from robopianist_amd import render
    key = (name, n_envs, precision, colorize_fingertips)
    if key not in _bare:
        _bare[key] = render.Renderer(rr.build_scene_variant(name), n_envs, precision=precision,
                                     colorize_fingertips=colorize_fingertips)
    return _bare[key]


def _dev(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device="cuda").contiguous()


def _real(precision):
    return torch.float32 if precision == 32 else torch.float64


def _as_held(x, precision):
    """x as the renderer of this precision reads it: the reference of a precision-32 image gets the rounded numbers."""
    return rr.rounded_to_float32(x) if precision == 32 else x


@pytest.mark.parametrize("precision", (64, 32))
@pytest.mark.parametrize("case", range(len(rr.wide_case_ids())), ids=rr.wide_case_ids())
def test_wide_cases_match_the_reference(case, precision):
    """Env 1 of a batch of two (env 0: the zero pose, no offset) against the reference: rgb, depth and segmentation."""
    name, q, off, cam, h, w, krgb, tips = rr.wide_cases()[case]
    r = _renderer(name, 2, precision, tips)
    nv = int(rr.build_scene_variant(name).model.nv)
    qpos = _dev(np.stack([np.zeros(nv), q]), _real(precision))
    toff = None if off is None else _dev(np.stack([np.zeros((2, 3)), off]), _real(precision))
    kr = None
    if krgb is not None:
        kr = rr.base_key_rgb(2); kr[1] = krgb
        kr = _dev(kr, torch.uint8)
    out = r.render(qpos, h, w, cam, tree_offset=toff, key_rgb=kr, rgb=True, depth=True, segmentation=True)
    torch.cuda.synchronize()
    got = tuple(_np(x)[1].copy() for x in out)
    assert got[0].dtype == np.uint8 and got[1].dtype == np.float32 and got[2].dtype == np.int32
    kw = dict(key_rgb=krgb, colorize_fingertips=tips) if krgb is not None else {}
    ref = rr.reference_for(name, _as_held(q, precision), cam, offsets=_as_held(off, precision), height=h, width=w, **kw)
    rr.compare_images(got, ref, label=f"gpu fp{precision} {rr.wide_case_ids()[case]}")


@pytest.mark.parametrize("case", range(len(rr.SCENES)), ids=rr.SCENES)
def test_images_match_the_reference_fp32(case):
    """test_images_match_the_reference through the fp32 engine: rp_render_frames_kernel<float>'s frames, as images."""
    name, pose, q = rr.image_cases()[case]
    phys = _physics(name, 2, precision=32)
    _set_qpos(phys, np.stack([q, q]))
    for cam in rr.CAMERAS:
        rgb = _np(phys.render(rr.H, rr.W, cam))[1].copy()
        depth = _np(phys.render(rr.H, rr.W, cam, depth=True))[1].copy()
        seg = _np(phys.render(rr.H, rr.W, cam, segmentation=True))[1].copy()
        rr.compare_images((rgb, depth, seg), rr.reference_for(name, rr.rounded_to_float32(q), cam),
                          label=f"gpu fp32 {name}/{pose}/{cam}")


def _fill_markers(bufs):
    bufs[0].fill_(7); bufs[1].fill_(-3.0); bufs[2].fill_(-9)


def _at_markers(bufs, rows):
    return bool((bufs[0][rows] == 7).all()) and bool((bufs[1][rows] == -3.0).all()) and bool((bufs[2][rows] == -9).all())


def test_mixed_batch_matches_the_reference_per_env():
    """Five envs, each with its own pose, tree offsets and key colours, fingertip colours on: every env against THE
    REFERENCE of its own inputs; then the window env_first = 2, env_count = 3 into marker-filled buffers."""
    q, off, krgb = rr.mixed_batch()
    E = rr.MIXED_ENVS
    r = _renderer("capsule", E, 64, True)
    qpos, toff, kr = _dev(q, torch.float64), _dev(off, torch.float64), _dev(krgb, torch.uint8)
    full = [x.clone() for x in r.render(qpos, rr.H, rr.W, "back", tree_offset=toff, key_rgb=kr, rgb=True, depth=True,
                                        segmentation=True)]
    for e in range(E):
        ref = rr.reference_for("capsule", q[e], "back", offsets=off[e], key_rgb=krgb[e], colorize_fingertips=True)
        rr.compare_images(tuple(_np(x[e]) for x in full), ref, label=f"gpu mixed batch env {e}")
    assert not torch.equal(full[2][0], full[2][1])
    bufs = r.outputs(rr.H, rr.W)
    _fill_markers(bufs)
    r.render(qpos, rr.H, rr.W, "back", tree_offset=toff, key_rgb=kr, rgb=True, depth=True, segmentation=True,
             env_first=2, env_count=3)
    torch.cuda.synchronize()
    assert _at_markers(bufs, slice(0, 2)), "the window wrote outside its envs"
    for b, f in zip(bufs, full):
        assert torch.equal(b[2:], f[2:]), "an env of the window differs from the full render"


GUARD = 4096
MARK = 0xA5


@pytest.mark.parametrize("h,w", ((15, 17), (16, 16), (1, 1), (29, 43)), ids=lambda v: str(v))
def test_nothing_outside_the_outputs_is_written(h, w):
    """rp_render into caller-owned buffers with 4096 marker bytes before and after each: H W = 255, 256, 1 and 1247, the
    full batch of three and the window of the last env, every output alone and all three."""
    from robopianist_amd import render
    E = 3
    m = rr.build_scene_variant("capsule").model
    r = _renderer("capsule", E)
    qpos = _dev(np.stack([rr.random_pose(m, 20 + e) for e in range(E)]), torch.float64)
    want = [x.clone() for x in r.render(qpos, h, w, "back", rgb=True, depth=True, segmentation=True)]
    want = [x.reshape(E, -1).view(torch.uint8) for x in want]          # [E][bytes of one env]
    stream = torch.cuda.current_stream().cuda_stream

    def run(first, count, outputs):
        bufs = [torch.full((2 * GUARD + E * wt.shape[1],), MARK, dtype=torch.uint8, device="cuda") for wt in want]
        ptr = [b.data_ptr() + GUARD if k in outputs else None for k, b in enumerate(bufs)]
        a = render.make_args("back", h, w, first, count, qpos=qpos.data_ptr(), rgb=ptr[0], depth=ptr[1],
                             segmentation=ptr[2], hip_stream=stream)
        assert r.render_raw(a) == 0, r.last_error()
        torch.cuda.synchronize()
        for k, (b, wt) in enumerate(zip(bufs, want)):
            what = f"{('rgb', 'depth', 'segmentation')[k]}, envs [{first}, {first + count}), outputs {outputs}"
            assert bool((b[:GUARD] == MARK).all()) and bool((b[-GUARD:] == MARK).all()), f"guard bytes overwritten: {what}"
            body = b[GUARD:-GUARD].view(E, -1)
            if k not in outputs:
                assert bool((body == MARK).all()), f"an output that was not asked for was written: {what}"
                continue
            for e in range(E):
                if first <= e < first + count:
                    assert torch.equal(body[e], wt[e]), f"env {e} differs from the renderer's own buffers: {what}"
                else:
                    assert bool((body[e] == MARK).all()), f"env {e} lies outside the window and was written: {what}"
        return bufs
    for first, count in ((0, E), (E - 1, 1)):
        for outputs in ((0,), (1,), (2,)):
            run(first, count, outputs)
        a, b = run(first, count, (0, 1, 2)), run(first, count, (0, 1, 2))
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "two identical calls differ"


BIG_E = 65540                       # 65535 + 5: rp_render cuts the call in two launches of rp_render_kernel
# the smallest of 1 x 1 .. 5 x 7 from closeup / back / free / topdown at which the reference shows >= 3 ids at all four
# poses (6 to 8), tells every two poses apart, shows the tree offset, and keeps every id when the camera is moved by
# 0.1 mm: no pixel sits on a silhouette, which 15 pixels and the 1 % cap leave no room for
BIG_H, BIG_W, BIG_CAMERA = 3, 5, "closeup"


def test_more_envs_than_a_grids_y_extent():
    """65540 envs, env e at pose e % 4 of four (e % 4 == 3 with a tree offset), 15 pixels each.  Envs 0..3 against the
    reference; every other env against env e % 4 on the device; then the window env_first = 3, env_count = 65537, whose
    second launch holds two envs."""
    from robopianist_amd import render
    si = rr.build_scene_variant("capsule")
    m = si.model
    assert BIG_E % 4 == 0 and BIG_E > 65535 + 3
    poses = np.stack([rr.random_pose(m, 30 + i) for i in range(4)])
    offs = np.zeros((4, 2, 3)); offs[3] = rr.WIDE_OFFSETS
    refs = [rr.reference_for("capsule", poses[i], BIG_CAMERA, offsets=offs[i] if i == 3 else None, height=BIG_H, width=BIG_W)
            for i in range(4)]
    assert all(len(np.unique(ref[2])) >= 3 for ref in refs)
    assert all(not np.array_equal(refs[a][2], refs[b][2]) for a in range(4) for b in range(a))
    assert not np.array_equal(refs[3][2], rr.reference_for("capsule", poses[3], BIG_CAMERA, height=BIG_H, width=BIG_W)[2])
    r = render.Renderer(si, BIG_E)
    qpos = _dev(poses, torch.float64).repeat(BIG_E // 4, 1)
    toff = _dev(offs, torch.float64).repeat(BIG_E // 4, 1, 1)
    kw = dict(tree_offset=toff, rgb=True, depth=True, segmentation=True)
    full = [x.clone() for x in r.render(qpos, BIG_H, BIG_W, BIG_CAMERA, **kw)]
    torch.cuda.synchronize()
    for i in range(4):
        rr.compare_images(tuple(_np(x[i]) for x in full), refs[i], label=f"gpu {BIG_E} envs, env {i}")
    for x, what in zip(full, ("rgb", "depth", "segmentation")):
        by_pose = x.view((BIG_E // 4, 4) + tuple(x.shape[1:]))
        assert torch.equal(by_pose, by_pose[:1].expand_as(by_pose)), f"{what}: an env differs from env e % 4"
    bufs = r.outputs(BIG_H, BIG_W)
    _fill_markers(bufs)
    r.render(qpos, BIG_H, BIG_W, BIG_CAMERA, env_first=3, env_count=BIG_E - 3, **kw)
    torch.cuda.synchronize()
    assert _at_markers(bufs, slice(0, 3)), "the window wrote outside its envs"
    for b, f, what in zip(bufs, full, ("rgb", "depth", "segmentation")):
        assert torch.equal(b[3:], f[3:]), f"{what}: an env of the window differs from the full render"


def test_render_on_another_stream():
    """hip_stream: qpos is filled on a side stream and rendered there; after that stream is synchronised the outputs equal
    the current-stream render, and geom_frames() (which waits for the LAST render's stream) returns the same frames."""
    m = rr.build_scene_variant("capsule").model
    r = _renderer("capsule", 2)
    pose_a = np.stack([rr.random_pose(m, 50), rr.random_pose(m, 51)])
    pose_b = np.stack([rr.random_pose(m, 52), rr.random_pose(m, 53)])
    kw = dict(rgb=True, depth=True, segmentation=True)
    want, frames = {}, {}
    for name, pose in (("a", pose_a), ("b", pose_b)):
        out = r.render(_dev(pose, torch.float64), rr.H, rr.W, "back", **kw)
        torch.cuda.synchronize()
        want[name] = [x.clone() for x in out]
        frames[name] = r.geom_frames()
    assert not torch.equal(want["a"][2], want["b"][2])              # (the buffers now hold b)
    side = torch.cuda.Stream()
    host_a, host_b = torch.as_tensor(pose_a).pin_memory(), torch.as_tensor(pose_b).pin_memory()
    qpos = torch.zeros((2, int(m.nv)), dtype=torch.float64, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qpos.copy_(host_a, non_blocking=True)
    out = r.render(qpos, rr.H, rr.W, "back", hip_stream=side.cuda_stream, **kw)
    side.synchronize()
    for x, y in zip(out, want["a"]):
        assert torch.equal(x, y), "the side-stream render differs from the current-stream render"
    got = r.geom_frames()
    assert np.array_equal(got[0], frames["a"][0]) and np.array_equal(got[1], frames["a"][1])
    # once more without synchronising: geom_frames() alone has to wait for the side stream
    with torch.cuda.stream(side):
        qpos.copy_(host_b, non_blocking=True)
    r.render(qpos, rr.H, rr.W, "back", hip_stream=side.cuda_stream, **kw)
    got = r.geom_frames()
    assert np.array_equal(got[0], frames["b"][0]) and np.array_equal(got[1], frames["b"][1])
    side.synchronize()
    for x, y in zip(r.outputs(rr.H, rr.W), want["b"]):
        assert torch.equal(x, y)
    r.render(qpos, rr.H, rr.W, "back", **kw)      # (leave the shared renderer on the current stream)
    torch.cuda.synchronize()
