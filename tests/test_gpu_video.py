"""The JPEG encoder on the device (librp_video.so) against the numpy restatement of the byte stream
(tests/video_reference.py), byte for byte; physics.render_jpeg and PianoSoundVideoWrapper end to end."""

import ctypes
import io
import os
import struct
import warnings

import numpy as np
import pytest
import torch

import video_reference as vr
from robopianist_amd import video

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda", 0)


def _encode_group(H, W, quality, cases, **kw):
    """One encoder, the group's images as one batch; (encoder, bytes, length) with the outputs on the host."""
    enc = video.Encoder(H, W, len(cases), quality=quality)
    rgb = torch.as_tensor(np.stack([vr.case_image(c) for c in cases]), device=_dev())
    out, length = enc.encode(rgb, **kw)
    torch.cuda.synchronize()
    return enc, out.cpu().numpy(), length.cpu().numpy()


def test_every_case_equals_the_restatement():
    """The whole case list, grouped into batches of one size and quality: frames of one batch differ in content and
    hence in length."""
    mixed = 0
    for (H, W, quality), cases in vr.groups().items():
        enc, out, length = _encode_group(H, W, quality, cases)
        assert enc.max_bytes == vr.max_bytes(H, W, quality) and enc.header == vr.header(H, W, quality)
        mixed += len(set(length.tolist())) > 1
        for f, case in enumerate(cases):
            want, _ = vr.case_reference(case)
            n = int(length[f])
            assert n == len(want), f"{vr.case_id(case)}: length {n}, the restatement has {len(want)}"
            got = out[f, :n].tobytes()
            if got != want:
                first = next(i for i in range(n) if got[i] != want[i])
                raise AssertionError(f"{vr.case_id(case)}: first differing byte at {first} of {n} (header {len(enc.header)})")
            assert not out[f, n:].any(), f"{vr.case_id(case)}: bytes past the file were written"
    assert mixed >= 3, "no batch with frames of different lengths: the compaction is not exercised"


def test_two_runs_are_bitwise_equal_and_the_window_leaves_other_rows_alone():
    cases = [c for c in vr.case_list() if c[1] == (30, 44) and c[2] == 90]
    assert len(cases) >= 5
    enc = video.Encoder(30, 44, len(cases), quality=90)
    rgb = torch.as_tensor(np.stack([vr.case_image(c) for c in cases]), device=_dev())
    out, length = enc.encode(rgb)
    first = (out.clone(), length.clone())
    out.zero_(); length.zero_()
    enc.encode(rgb)
    torch.cuda.synchronize()
    assert torch.equal(out, first[0]) and torch.equal(length, first[1])
    # a window of two frames in the middle: the other rows keep the marker they are given here
    out.fill_(0xA5); length.fill_(-7)
    enc.encode(rgb, frame_first=2, frame_count=2)
    torch.cuda.synchronize()
    o, n = out.cpu().numpy(), length.cpu().numpy()
    for f in range(len(cases)):
        if f in (2, 3):
            want, _ = vr.case_reference(cases[f])
            assert n[f] == len(want) and o[f, :n[f]].tobytes() == want and (o[f, n[f]:] == 0xA5).all()
        else:
            assert n[f] == -7 and (o[f] == 0xA5).all()


def test_a_small_cap_reports_the_need_and_writes_nothing_past_it():
    case = ("noise", (80, 176), 100, 1)
    want, _ = vr.case_reference(case)
    enc = video.Encoder(80, 176, 1, quality=100)
    rgb = torch.as_tensor(np.array(vr.case_image(case))[None], device=_dev())
    for cap in (len(want) - 1, len(want) // 2, 300, 1):
        guard = torch.full((cap + 4096,), 0x5A, dtype=torch.uint8, device=_dev())
        length = torch.zeros(1, dtype=torch.int32, device=_dev())
        a = video.make_args(0, 1, cap, rgb=rgb.data_ptr(), out_bytes=guard.data_ptr(), length=length.data_ptr(),
                            hip_stream=torch.cuda.current_stream().cuda_stream)
        assert enc.encode_raw(a) == 0, enc.last_error()
        torch.cuda.synchronize()
        g = guard.cpu().numpy()
        assert int(length[0]) == -len(want)
        assert g[:cap].tobytes() == want[:cap] and (g[cap:] == 0x5A).all(), f"cap {cap}"
    with pytest.raises(video.VideoError, match="needs"):
        enc.frames(rgb, bytes_cap=300)
    # exactly enough is enough
    out, length = enc.encode(rgb, bytes_cap=len(want))
    assert int(length[0]) == len(want) and out[0].cpu().numpy().tobytes() == want


def _awkward_caps(case):
    """{what: bytes_cap} from the restatement's bytes alone: the caps that fall on the bytes a store of two (a 0xFF
    and its stuffed zero, the two bytes of a marker) or a store by another lane or kernel (the header, a seam byte, a
    segment placed in a later round of the layout) can get wrong."""
    want, st = vr.case_reference(case)
    head = len(vr.header(case[1][0], case[1][1], case[2]))
    seg_at, zeros = st["seg_at"], st["stuffed_at"]
    caps = {"header - 1": head - 1, "header": head, "header + 1": head + 1}
    assert zeros, "no stuffed byte in this case"
    for name, z in (("first", zeros[0]), ("last", zeros[-1])):
        assert want[z - 1] == 0xFF and want[z] == 0
        caps[f"{name} stuffed zero"] = z            # the 0xFF is written, its zero is not
        caps[f"{name} stuffed zero + 1"] = z + 1
    if st["group_edge_at"]:
        caps["stuffed zero of lane 63"] = st["group_edge_at"][0] + 1
    # the markers: a restart marker where there is one, the end of image where the frame is one segment
    # the markers: restart markers 0 and 7 (after which the count wraps) and the one before segment 64; the end of image
    for s in sorted({0, 7, 63, st["segments"] - 1}):
        if s < st["segments"]:
            m = seg_at[s + 1] - 2
            assert want[m] == 0xFF and want[m + 1] == (0xD9 if s == st["segments"] - 1 else 0xD0 + s % 8)
            caps[f"marker of segment {s}, second byte"] = m + 1   # the 0xFF is written, the number is not
            caps[f"marker of segment {s}, first byte"] = m
    for k, at in enumerate(st["seam_at"]):
        caps[f"seam byte {k}"] = at
        caps[f"seam byte {k} + 1"] = at + 1
    for k, z in enumerate(st["seam_prev_at"]):
        assert want[z - 1] == 0xFF and want[z] == 0
        caps[f"stuffed zero {k} that ends a chunk"] = z
        caps[f"stuffed zero {k} that ends a chunk, + 1"] = z + 1
    if st["segments"] > 64:
        caps["first byte of segment 64"] = seg_at[64]
        caps["first byte of segment 64, + 1"] = seg_at[64] + 1
    assert all(0 < c < len(want) for c in caps.values())
    return caps


AWKWARD_CASES = (vr.SEAM_FF_CASE, vr.SEAM_PREV_FF_CASE, ("noise", (520, 8), 100, 0))


@pytest.mark.parametrize("case", AWKWARD_CASES, ids=vr.case_id)
def test_caps_on_the_awkward_bytes(case):
    """Every cap of _awkward_caps, alone and as the middle row of three (frame_first = 1, frame_count = 1): the need is
    reported, the row holds the file up to the cap, and nothing else changes: neither the guard behind the row, nor the
    neighbouring rows, nor their lengths."""
    want, st = vr.case_reference(case)
    (H, W), quality = case[1], case[2]
    caps = _awkward_caps(case)
    if case == vr.SEAM_FF_CASE:
        assert st["seam_ff"] and any(want[at] == 0xFF and caps[f"seam byte {k} + 1"] == at + 1 for k, at in enumerate(st["seam_at"]))
    elif case == vr.SEAM_PREV_FF_CASE:
        assert "stuffed zero 0 that ends a chunk" in caps and "marker of segment 7, second byte" in caps
    else:
        assert st["segments"] == 65 and "first byte of segment 64" in caps and "stuffed zero of lane 63" in caps
    image = np.array(vr.case_image(case))
    one = video.Encoder(H, W, 1, quality=quality)
    three = video.Encoder(H, W, 3, quality=quality)
    rgb1 = torch.as_tensor(image[None], device=_dev())
    rgb3 = torch.as_tensor(np.stack([vr.noise(H, W, 101), image, vr.noise(H, W, 102)]), device=_dev())
    stream = torch.cuda.current_stream().cuda_stream
    for what, cap in caps.items():
        guard = torch.full((cap + 4096,), 0x5A, dtype=torch.uint8, device=_dev())
        length = torch.zeros(1, dtype=torch.int32, device=_dev())
        a = video.make_args(0, 1, cap, rgb=rgb1.data_ptr(), out_bytes=guard.data_ptr(), length=length.data_ptr(), hip_stream=stream)
        assert one.encode_raw(a) == 0, one.last_error()
        torch.cuda.synchronize()
        g = guard.cpu().numpy()
        assert int(length[0]) == -len(want), what
        assert g[:cap].tobytes() == want[:cap], f"{what}: cap {cap}"
        assert (g[cap:] == 0x5A).all(), f"{what}: cap {cap}, written at {cap + int(np.flatnonzero(g[cap:] != 0x5A)[0])}"
        # the middle row of three
        guard = torch.full((3 * cap + 4096,), 0x5A, dtype=torch.uint8, device=_dev())
        length = torch.full((3,), -7, dtype=torch.int32, device=_dev())
        a = video.make_args(1, 1, cap, rgb=rgb3.data_ptr(), out_bytes=guard.data_ptr(), length=length.data_ptr(), hip_stream=stream)
        assert three.encode_raw(a) == 0, three.last_error()
        torch.cuda.synchronize()
        g = guard.cpu().numpy()
        assert length.cpu().tolist() == [-7, -len(want), -7], what
        assert g[cap:2 * cap].tobytes() == want[:cap], f"{what}: cap {cap}, row 1 of 3"
        assert (g[:cap] == 0x5A).all() and (g[2 * cap:] == 0x5A).all(), f"{what}: cap {cap}, a neighbouring row was written"


def test_a_mixed_batch_across_two_rounds_of_segments():
    """Four frames of 65 segments in one call, all of different lengths: each frame's segments 64 are placed by its own
    carried sum.  Then a window against poisoned rows, and a second run."""
    cases = [("flat", (520, 8), 90, 0), ("noise", (520, 8), 90, 0), ("noise", (520, 8), 90, 7), ("block_checkerboard", (520, 8), 90, 0)]
    wants = [vr.case_reference(c)[0] for c in cases]
    assert len({len(w) for w in wants}) == 4
    enc = video.Encoder(520, 8, 4, quality=90)
    assert enc._L.rp_video_dim(enc._h, b"segments") == 65 and enc._L.rp_video_dim(enc._h, b"chunk_blocks") == vr.CHUNK_BLOCKS
    rgb = torch.as_tensor(np.stack([vr.case_image(c) for c in cases]), device=_dev())
    out, length = enc.encode(rgb)
    torch.cuda.synchronize()
    first = (out.clone(), length.clone())
    o, n = out.cpu().numpy(), length.cpu().numpy()
    for f, want in enumerate(wants):
        assert n[f] == len(want), f"frame {f}: length {n[f]}, the restatement has {len(want)}"
        got = o[f, :n[f]].tobytes()
        if got != want:
            at = next(i for i in range(n[f]) if got[i] != want[i])
            raise AssertionError(f"frame {f}: first differing byte at {at} of {n[f]} (header {len(enc.header)})")
        assert not o[f, n[f]:].any()
    out.zero_(); length.zero_()
    enc.encode(rgb)
    torch.cuda.synchronize()
    assert torch.equal(out, first[0]) and torch.equal(length, first[1])
    out.fill_(0xA5); length.fill_(-7)
    enc.encode(rgb, frame_first=1, frame_count=2)
    torch.cuda.synchronize()
    o, n = out.cpu().numpy(), length.cpu().numpy()
    for f, want in enumerate(wants):
        if f in (1, 2):
            assert n[f] == len(want) and o[f, :n[f]].tobytes() == want and (o[f, n[f]:] == 0xA5).all()
        else:
            assert n[f] == -7 and (o[f] == 0xA5).all()


def test_rows_beyond_four_gib_of_output():
    """8 x 344 at quality 100 with bytes_cap = max_bytes (54,167): 79,300 frames are 2^32 bytes of rows and eight rows
    more, so a row offset formed in 32 bits puts the later frames on top of the first ones.  Frame f is image f % 7 of
    a bank of seven; every length is compared on the device, and the frames at both ends and on either side of the
    2^32th byte byte for byte.  (`rgb` is 0.65 GB and the coefficients 1.3 GB: only `bytes` crosses 2^32.  On an
    MI355X the test takes 0.3 s.)"""
    import time
    H, W, quality = 8, 344, 100
    cap = vr.max_bytes(H, W, quality)
    N = -(-2 ** 32 // cap) + 8
    bank = [vr.noise(H, W, 1), vr.noise(H, W, 2), vr.saturated(H, W, 0), vr.block_checkerboard(H, W), vr.flat(H, W),
            vr.rendered_like(H, W), vr.gradient(H, W)]
    wants = [vr.encode(img, quality) for img in bank]
    assert len({len(w) for w in wants}) == 7
    below = (2 ** 32 - 1) // cap            # the last row that starts below 2^32
    assert below * cap < 2 ** 32 <= (below + 1) * cap and below + 1 < N - 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enc = video.Encoder(H, W, N, quality=quality)
    assert enc.max_bytes == cap
    index = torch.arange(N, device=_dev()) % 7
    rgb = torch.as_tensor(np.stack(bank), device=_dev())[index].contiguous()
    out, length = enc.encode(rgb)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    try:
        assert out.shape == (N, cap) and out.numel() > 2 ** 32
        table = torch.tensor([len(w) for w in wants], dtype=torch.int32, device=_dev())
        wrong = torch.nonzero(length != table[index]).flatten()
        assert wrong.numel() == 0, f"{wrong.numel()} wrong lengths, the first at frame {int(wrong[0])}"
        for f in (0, 1, below, below + 1, N - 1):
            want = wants[f % 7]
            row = out[f].cpu().numpy()
            assert row[:len(want)].tobytes() == want, f"frame {f}"
            assert not row[len(want):].any(), f"frame {f}: bytes past the file were written"
    finally:
        del out, length, rgb
        enc._out.clear()
        del enc
        torch.cuda.empty_cache()
    print(f"{N} frames of {H} x {W}, rows of {cap} bytes: create, build rgb and encode took {t1 - t0:.3f} s, "
          f"the whole test {time.perf_counter() - t0:.3f} s")


def test_refusals_launch_nothing():
    for bad in (dict(height=0), dict(width=0), dict(quality=0), dict(quality=101), dict(max_frames=0), dict(height=65536)):
        kw = dict(height=8, width=8, max_frames=1, quality=90)
        kw.update(bad)
        with pytest.raises(video.VideoError):
            video.Encoder(**kw)
    enc = video.Encoder(8, 8, 4, quality=90)
    rgb = torch.as_tensor(np.stack([vr.noise(8, 8, s) for s in range(4)]), device=_dev())
    out, length = enc.outputs()
    out.fill_(0xA5); length.fill_(-7)
    torch.cuda.synchronize()

    def args(**kw):
        a = video.make_args(0, 4, out.shape[1], rgb=rgb.data_ptr(), out_bytes=out.data_ptr(), length=length.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for kw in (dict(struct_size=ctypes.sizeof(video.EncodeArgs) - 8), dict(frame_first=-1), dict(frame_count=0),
               dict(frame_first=1, frame_count=4), dict(frame_first=4, frame_count=1), dict(bytes_cap=0),
               dict(rgb=None), dict(bytes=None), dict(length=None)):
        assert enc.encode_raw(args(**kw)) != 0, kw
        assert enc.last_error()
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and (length == -7).all()
    with pytest.raises(video.VideoError, match="shape"):
        enc.encode(rgb[:3])
    assert enc.encode_raw(args()) == 0
    torch.cuda.synchronize()
    assert (length > 0).all()


def test_many_small_frames_in_one_call():
    """70 000 frames of 1 x 1 (more than a grid's y or z dimension takes; the encoder indexes its grids by x alone):
    frame f is the flat colour (f % 251, f % 241, f % 239), so 251 x 241 x 239 distinct files cannot repeat by
    accident; every 997th frame and the last are checked against the restatement, and all lengths."""
    N = 70000
    f = np.arange(N)
    rgb = np.stack([f % 251, f % 241, f % 239], -1).astype(np.uint8).reshape(N, 1, 1, 3)
    enc = video.Encoder(1, 1, N, quality=75)
    out, length = enc.encode(torch.as_tensor(rgb, device=_dev()))
    torch.cuda.synchronize()
    n = length.cpu().numpy()
    head = len(enc.header)
    assert (n > head).all() and (n <= enc.max_bytes).all()
    for i in list(range(0, N, 997)) + [N - 1]:
        want = vr.encode(rgb[i], 75)
        assert n[i] == len(want) and out[i, :n[i]].cpu().numpy().tobytes() == want, f"frame {i}"


def _scene_env(n_envs, **kw):
    from robopianist_amd import suite
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", n_envs=n_envs, seed=11,
                          task_kwargs=dict(trim_silence=True, control_timestep=0.05, gravity_compensation=True,
                                           primitive_fingertip_collisions=True), **kw)


def test_render_jpeg_equals_the_restatement_of_the_rendered_image():
    env = _scene_env(2)
    env.reset()
    physics = env.physics
    # the two envs differ: env 1's keys are coloured
    key_rgb = torch.zeros((2, 88, 3), dtype=torch.uint8, device=physics.device)
    key_rgb[0] = 230
    key_rgb[1, ::2] = torch.tensor([30, 200, 60], dtype=torch.uint8, device=physics.device)
    files = physics.render_jpeg(30, 44, "piano/back", quality=90, key_rgb=key_rgb)
    images = physics.render(30, 44, "piano/back", key_rgb=key_rgb).cpu().numpy()
    assert len(files) == 2 and files[0] != files[1]
    for e in range(2):
        assert files[e] == vr.encode(images[e], 90)
        im = vr.decode(files[e])
        assert im.size == (44, 30) and im.mode == "RGB"
        assert vr.psnr(np.asarray(im), images[e]) > 25.0
    only = physics.render_jpeg(30, 44, "piano/back", quality=90, key_rgb=key_rgb, envs=[1])
    assert only == [files[1]]
    assert physics.render_jpeg(30, 44, "piano/back", quality=30, key_rgb=key_rgb)[0] == vr.encode(images[0], 30)


def test_render_jpeg_of_a_tall_frame_equals_the_restatement():
    """The caller's route through more than 64 segments: 520 x 8, two envs with different keys."""
    env = _scene_env(2)
    env.reset()
    physics = env.physics
    key_rgb = torch.zeros((2, 88, 3), dtype=torch.uint8, device=physics.device)
    key_rgb[0] = 230
    key_rgb[1, ::2] = torch.tensor([30, 200, 60], dtype=torch.uint8, device=physics.device)
    files = physics.render_jpeg(520, 8, "piano/back", quality=90, key_rgb=key_rgb)
    images = physics.render(520, 8, "piano/back", key_rgb=key_rgb).cpu().numpy()
    assert len(files) == 2 and images.shape == (2, 520, 8, 3)
    for e in range(2):
        st = {}
        assert files[e] == vr.encode(images[e], 90, st), f"env {e}"
        assert st["segments"] == 65
        im = vr.decode(files[e])
        assert im.size == (8, 520) and im.mode == "RGB"
        assert vr.psnr(np.asarray(im), images[e]) > 25.0


def _riff_chunks(data):
    """[(fourcc, payload)] of the movi list, and the stream count of the header."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    chunks, streams, i = [], 0, 12
    while i < len(data):
        fourcc, n = data[i:i + 4], struct.unpack("<I", data[i + 4:i + 8])[0]
        if fourcc == b"LIST" and data[i + 8:i + 12] == b"hdrl":
            streams = data[i:i + 8 + n].count(b"strh")
        if fourcc == b"LIST" and data[i + 8:i + 12] == b"movi":
            j = i + 12
            while j < i + 8 + n:
                m = struct.unpack("<I", data[j + 4:j + 8])[0]
                chunks.append((data[j:j + 4], data[j + 8:j + 8 + m]))
                j += 8 + m + (m & 1)
        i += 8 + n + (n & 1)
    return chunks, streams


def test_sound_video_wrapper_end_to_end(tmp_path):
    """Three envs, record_envs=(2, 1): env 1 replays the Twinkle actions (it plays notes), env 2 holds zeros (silent),
    env 0 is not tracked.  A twin PianoSoundWrapper on the same environment writes the .wav of the same episode."""
    import wave
    from robopianist_amd.wrappers import PianoSoundVideoWrapper, PianoSoundWrapper
    actions = np.load(os.path.join(ROOT, "tests", "golden", "twinkle_twinkle_actions.npy"))
    base = _scene_env(3, record_key_trace=True)
    dev, dtype = base.physics.device, base.physics.dtype
    sound = PianoSoundWrapper(base, tmp_path / "wav", record_envs=(2, 1))
    env = PianoSoundVideoWrapper(sound, tmp_path / "avi", record_envs=(2, 1), camera_id="piano/back", height=48, width=64,
                                 quality=90)
    task = base.task
    spec = base.action_spec()
    zero = torch.zeros(tuple(spec.shape), dtype=dtype, device=dev)
    lo = torch.as_tensor(spec.minimum, dtype=dtype, device=dev)
    half = 0.5 * (torch.as_tensor(spec.maximum, dtype=dtype, device=dev) - lo)
    # (the recorded actions are canonical, in [-1, 1]: mapped onto the spec as CanonicalSpecWrapper does)
    played = lo + (torch.as_tensor(actions, dtype=dtype, device=dev) + 1.0) * half

    def beside():
        img = base.physics.render(48, 64, "piano/back", key_rgb=task.key_rgb(base.physics),
                                  colorize_fingertips=bool(getattr(task, "colorize_fingertips", False)))
        return img[1:3].cpu().numpy().copy()

    def episode():
        frames = []
        for t in range(len(actions) + 5):
            ts = env.step(torch.stack([zero, played[min(t, len(actions) - 1)], zero]))
            frames.append(beside())
            if bool(ts.last().all()):
                return frames
        raise AssertionError("the episode did not end")

    env.reset()
    first = [beside()] + episode()
    names = sorted(p.name for p in (tmp_path / "avi").iterdir())
    assert names == ["0001_00000.avi", "0002_00000.avi"] and sorted(p.name for p in env.written) == names
    assert sorted(p.name for p in (tmp_path / "wav").iterdir()) == ["0001_00000.wav"], "env 1 plays, env 2 is silent"
    for name, row in (("0001_00000.avi", 0), ("0002_00000.avi", 1)):
        chunks, streams = _riff_chunks((tmp_path / "avi" / name).read_bytes())
        pictures = [p for k, p in chunks if k == b"00dc"]
        assert len(pictures) == len(first), "one frame per step, the FIRST step's included"
        for t, p in enumerate(pictures):
            assert p == vr.encode(first[t][row], 90), f"{name}: frame {t}"
        assert vr.decode(pictures[-1]).size == (64, 48)
        sound_bytes = b"".join(p for k, p in chunks if k == b"01wb")
        if row == 0:
            with wave.open(str(tmp_path / "wav" / "0001_00000.wav"), "rb") as wf:
                want = wf.readframes(wf.getnframes())
            assert streams == 2 and sound_bytes == want and len(want) > 0
        else:
            assert streams == 1 and sound_bytes == b""
    assert any(f[0].tobytes() != first[0][0].tobytes() for f in first[1:]), "nothing moved: the frames show nothing"
    # a second episode: the step after LAST is FIRST, and its frame is the first of the new recording
    ts = env.step(torch.stack([zero, zero, zero]))
    assert bool(ts.first().all())
    second = [beside()] + episode()
    chunks, _ = _riff_chunks((tmp_path / "avi" / "0001_00001.avi").read_bytes())
    pictures = [p for k, p in chunks if k == b"00dc"]
    assert len(pictures) == len(second)
    for t in (0, 1, len(second) // 2, len(second) - 1):
        assert pictures[t] == vr.encode(second[t][0], 90), f"second episode: frame {t}"
