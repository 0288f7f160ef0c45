"""GPU tests of the camera renderer (include/render/rp_render.h, librp_render.so) and the pixel observation wrapper.

Images are 30 x 44 (H W = 1320 is no multiple of 256: the last workgroup of every image is partial), E <= 5.  The
numpy reference, the cases, the 1 % segmentation cap and the depth tolerance are the CPU suite's
(tests/render_reference.py: the reference in float32 against itself in float64 differs by 5.4969e-05 in depth on these
images; DEPTH_TOL = 4 x that = 2.1988e-04).
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
