"""The JPEG encoder without a GPU: the committed tables, the g++ build of csrc/rp_video.hpp against the numpy
restatement (tests/video_reference.py) byte for byte, what Pillow makes of the files, the ABI, and the AVI writer."""

import ctypes
import io
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import video_reference as vr
from robopianist_amd import video

ALL_CASES = vr.case_list()


def _host_file(case):
    hv = vr.HostVideo(case[1][0], case[1][1], 1, case[2])
    (data,), length = hv.frames(vr.case_image(case)[None])
    assert int(length[0]) == len(data)
    return data, hv


# ---- tables ----------------------------------------------------------------------------------------------------------
def test_the_committed_dct_integers_and_zigzag_equal_the_formula():
    L = vr.host_library()
    ci = np.array(L.rpvh_dct_integers()[:64]).reshape(8, 8)
    assert (ci == vr.dct_integers()).all()
    assert (ci[:, ::-1] == ci * np.array([1, -1] * 4)[:, None]).all(), "Ci[u][7-x] = (-1)^u Ci[u][x]: the kernels rely on it"
    assert (np.array(L.rpvh_zigzag()[:64]) == vr.zigzag()).all()
    assert L.rpvh_div_mismatches() == 0, "n / Q by multiplication is exact for every n < 2^16 and Q in 1..255"


def test_the_quantisation_tables_at_every_quality_equal_libjpegs():
    from PIL import Image
    img = np.zeros((8, 8, 3), np.uint8)
    for quality in range(1, 101):
        theirs = Image.open(io.BytesIO(vr.pillow_jpeg(img, quality=quality, subsampling=0))).quantization
        head = vr.HostVideo(8, 8, 1, quality).header
        ours, _ = vr.parse_tables(head + b"")
        # (Pillow reports the tables in natural order, the file stores them in zigzag order)
        natural = {k: [v[int(z)] for z in np.argsort(vr.zigzag())] for k, v in ours.items()}
        assert {k: list(v) for k, v in theirs.items()} == natural, f"quality {quality}"
        assert [list(map(int, q)) for q in vr.quant_tables(quality)] == [ours[0], ours[1]]


def test_the_huffman_tables_equal_the_dht_segments_of_a_libjpeg_file():
    theirs = vr.parse_tables(vr.pillow_jpeg(np.zeros((8, 8, 3), np.uint8), quality=75, subsampling=0))[1]
    ours = vr.parse_tables(vr.HostVideo(8, 8, 1, 75).header)[1]
    assert sorted(ours) == [0x00, 0x01, 0x10, 0x11] and ours == theirs


def test_the_header_is_the_restatements_and_in_the_defined_order():
    for (H, W, quality) in ((8, 8, 90), (1, 1, 1), (9, 17, 50), (80, 176, 100), (480, 640, 90)):
        hv = vr.HostVideo(H, W, 1, quality)
        assert hv.header == vr.header(H, W, quality)
        assert hv.max_bytes == vr.max_bytes(H, W, quality)
        markers = [m for m, _ in vr.parse_segments(hv.header)[0]]
        assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]


# ---- the host build against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=vr.case_id)
def test_host_build_equals_the_restatement_and_pillow_decodes_it(case):
    want, _ = vr.case_reference(case)
    got, hv = _host_file(case)
    assert got == want
    assert len(got) <= hv.max_bytes
    im = vr.decode(got)
    assert im.size == (case[1][1], case[1][0]) and im.mode == "RGB"
    if case[0] in ("flat", "block_checkerboard") and case[2] == 100:
        assert (np.asarray(im) == vr.case_image(case)).all(), "quality 100 keeps a flat or block-wise flat image exactly"
    if case in vr.TALL_CASES:
        # a decoder that is not ours follows the restart markers over 65 and 129 segments: one out of sequence, or a
        # segment out of place, and it decodes something else from there on (the floor is render_jpeg's)
        assert vr.psnr(np.asarray(im), vr.case_image(case)) > 25.0


def test_exact_decoding_cases_are_in_the_list():
    exact = [c for c in ALL_CASES if c[0] in ("flat", "block_checkerboard") and c[2] == 100]
    assert {c[0] for c in exact} == {"flat", "block_checkerboard"}


def test_the_cases_are_what_they_claim():
    stats = [vr.case_reference(c)[1] for c in ALL_CASES]
    assert any(s["zrl"] for s in stats), "no ZRL"
    assert any(s["no_eob"] for s in stats), "no block without EOB"
    assert max(s["max_dc_size"] for s in stats) == 11, "no DC difference of size 11"
    assert max(s["max_ac_size"] for s in stats) == 10, "no AC value of size 10"
    assert any(s["neg_dc"] for s in stats) and any(s["neg_ac"] for s in stats)
    assert any(s["stuffed"] for s in stats), "no stuffed 0xFF"
    assert any(s["stuffed_pad"] for s in stats), "no stuffed pad byte"
    assert vr.case_reference(vr.PAD_STUFF_CASE)[1]["stuffed_pad"] == 1
    blocks = {s["segment_blocks"] for s in stats}
    hv = vr.HostVideo(8, 8, 1, 90)
    chunk = hv._L.rpvh_dim(hv._h, b"chunk_blocks")
    assert chunk == 64 == vr.CHUNK_BLOCKS, "the restatement counts its seams with the library's chunk size"
    assert any(b > chunk for b in blocks) and any(b > 2 * chunk for b in blocks), "no segment longer than a chunk"
    assert chunk - 1 in blocks, "63 blocks: one short of a chunk (3 blocks per tile, so 64 itself cannot occur)"
    assert not any(b == chunk for b in blocks) and chunk % 3 != 0
    assert any(s["segments"] > 8 for s in stats), "no frame of more than 8 segments: the RST counter never wraps"
    # the extremes sit on the segments that cross a chunk, too
    long_noise = vr.case_reference(("noise", (80, 176), 100, 1))[1]
    assert long_noise["no_eob"] and long_noise["stuffed"] and long_noise["segments"] == 10
    # the layout's rounds of 64 segments: a second and a third round, and sizes that differ along the frame, so that a
    # segment placed by a wrong sum lands on other bytes
    assert any(s["segments"] > 64 for s in stats) and any(s["segments"] > 128 for s in stats)
    for case in vr.TALL_CASES:
        st = vr.case_reference(case)[1]
        sizes = np.diff(st["seg_at"])
        assert st["segments"] > 64 and len(sizes) == st["segments"]
        assert len(set(sizes.tolist())) > 4 and len(set(sizes[:64].tolist())) > 4, vr.case_id(case)
    assert {vr.case_reference(c)[1]["segments"] for c in vr.TALL_CASES} == {65, 129}
    assert max(s["chunks"] for s in stats) >= 7, "bits are carried six times in no case"
    assert any(s["chunks"] >= 7 and s["segments"] >= 3 for s in stats), "many chunks in many segments"
    # what can fall on a seam between two chunks
    for event in ("seam_ff", "seam_aligned", "seam_prev_ff", "group_edge_ff"):
        assert any(s[event] for s in stats), f"no case with {event}"
    assert vr.case_reference(vr.SEAM_FF_CASE)[1]["seam_ff"] == 1
    assert vr.case_reference(vr.SEAM_ALIGNED_CASE)[1]["seam_aligned"] == 1
    assert vr.case_reference(vr.SEAM_PREV_FF_CASE)[1]["seam_prev_ff"] == 1
    assert vr.case_reference(("noise", (80, 176), 100, 1))[1]["group_edge_ff"] == 7
    assert vr.search_seam_seed("seam_ff", (8, 344), 100, 8) == vr.SEAM_FF_CASE[3], "how the seed was found"
    assert vr.search_seam_seed("seam_aligned", (8, 344), 100, 8) == vr.SEAM_ALIGNED_CASE[3]
    assert vr.search_seam_seed("seam_prev_ff", (80, 176), 98, 12) == vr.SEAM_PREV_FF_CASE[3]
    # how full a chunk's bit buffer gets: the dense cases fill it further than anything before them, and furthest of all
    before = max(vr.case_reference(c)[1]["max_chunk_bits"] for c in vr.base_case_list())
    others = max(vr.case_reference(c)[1]["max_chunk_bits"] for c in ALL_CASES if c not in vr.DENSE_CASES)
    for case in vr.DENSE_CASES:
        st = vr.case_reference(case)[1]
        print(f"{vr.case_id(case)}: max_block_bits {st['max_block_bits']}, max_chunk_bits {st['max_chunk_bits']} "
              f"(before: {before}, the other cases: {others})")
        assert st["max_chunk_bits"] > before and st["max_chunk_bits"] > others
    assert max(s["max_block_bits"] for s in stats) == max(vr.case_reference(c)[1]["max_block_bits"] for c in vr.DENSE_CASES)


def test_fidelity_against_libjpeg():
    """PSNR of our stream, decoded by Pillow, against libjpeg's own encoding with the same tables (4:4:4).  libjpeg's
    default DCT is its own integer approximation (jfdctint), so the two differ by rounding either way.  The bound is
    max(0.1 dB, 2 x the restatement's worst deficit on these cases as this test measures it).  Measured with Pillow 12.2:
    the restatement is between 0.119 dB better (pixel checkerboard, quality 90) and 0.058 dB worse (noise, quality 90)
    than libjpeg, 0.052 dB worse at most on the rendered-like images; the bound is therefore 0.115 dB."""
    reference = vr.measure_fidelity(lambda img, q: vr.encode(img, q))
    worst_ref = max(reference.values())
    for k, v in reference.items():
        print(f"restatement {k}: deficit {v:+.4f} dB")
    print(f"restatement: worst deficit {worst_ref:+.4f} dB, best {min(reference.values()):+.4f} dB")
    bound = max(0.1, 2.0 * worst_ref)

    def host(img, q):
        (data,), _ = vr.HostVideo(img.shape[0], img.shape[1], 1, q).frames(img[None])
        return data
    ours = vr.measure_fidelity(host)
    print(f"host build: worst deficit {max(ours.values()):+.4f} dB (bound {bound:.4f} dB)")
    assert max(ours.values()) <= bound
    assert ours == reference


# ---- the call ----------------------------------------------------------------------------------------------------------
def _batch():
    cases = [c for c in ALL_CASES if c[1] == (30, 44) and c[2] == 90]
    return cases, np.stack([vr.case_image(c) for c in cases])


def test_a_batch_of_different_frames_and_the_window():
    cases, rgb = _batch()
    hv = vr.HostVideo(30, 44, len(cases), 90)
    files, length = hv.frames(rgb)
    assert files == [vr.case_reference(c)[0] for c in cases] and len(set(length.tolist())) > 1
    out = np.full((len(cases), hv.max_bytes), 0xA5, np.uint8)
    length = np.full(len(cases), -7, np.int32)
    assert hv.encode_into(rgb, out, length, frame_first=2, frame_count=2) == 0
    for f in range(len(cases)):
        if f in (2, 3):
            assert out[f, :length[f]].tobytes() == files[f] and (out[f, length[f]:] == 0xA5).all()
        else:
            assert length[f] == -7 and (out[f] == 0xA5).all()


def test_overflow_reports_the_need_and_leaves_the_rest_untouched():
    case = ("noise", (80, 176), 100, 1)
    want, _ = vr.case_reference(case)
    hv = vr.HostVideo(80, 176, 1, 100)
    rgb = np.ascontiguousarray(vr.case_image(case))
    for cap in (len(want) - 1, 300, 1):
        guard = np.full((1, cap + 64), 0x5A, np.uint8)
        length = np.zeros(1, np.int32)
        a = video.make_args(0, 1, cap, rgb=rgb.ctypes.data, out_bytes=guard.ctypes.data,
                            length=length.ctypes.data)
        assert hv._L.rpvh_encode(hv._h, ctypes.byref(a)) == 0
        assert length[0] == -len(want)
        assert guard[0, :cap].tobytes() == want[:cap] and (guard[0, cap:] == 0x5A).all()
    assert max(len(vr.case_reference(c)[0]) for c in ALL_CASES if c[1] == (80, 176)) <= hv.max_bytes


def test_max_bytes_bounds_every_case():
    for case in ALL_CASES:
        assert len(vr.case_reference(case)[0]) <= vr.max_bytes(case[1][0], case[1][1], case[2])


def test_refusals():
    L = vr.host_library()
    for kw in (dict(quality=0), dict(quality=101), dict(height=0), dict(width=0), dict(height=65536), dict(max_frames=0)):
        full = dict(height=8, width=8, max_frames=1, quality=90)
        full.update(kw)
        h = ctypes.c_void_p()
        assert L.rpvh_create(full["height"], full["width"], full["max_frames"], full["quality"], 0, ctypes.byref(h)) != 0, kw
        assert L.rpvh_last_error()
    hv = vr.HostVideo(8, 8, 4, 90)
    rgb = np.stack([vr.noise(8, 8, s) for s in range(4)])
    out = np.full((4, hv.max_bytes), 0xA5, np.uint8)
    length = np.full(4, -7, np.int32)
    assert hv.encode_into(rgb, out, length, struct_size=ctypes.sizeof(video.EncodeArgs) + 8) != 0
    assert "struct_size" in hv.last_error()
    for first, count in ((-1, 1), (0, 0), (1, 4), (4, 1), (0, 5)):
        assert hv.encode_into(rgb, out, length, frame_first=first, frame_count=count) != 0, (first, count)
        assert "window" in hv.last_error()
    assert hv.encode_into(rgb, out[:, :0], length) != 0
    assert (out == 0xA5).all() and (length == -7).all()


def _struct_fields(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    names = []
    for stmt in body.split(";"):
        for part in stmt.strip().split(",") if stmt.strip() else []:
            names.append(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", re.sub(r"\[\d+\]", "", part))[-1])
    return names


def test_video_abi_struct_and_symbols_match_the_header():
    src = open(os.path.join(vr.ROOT, "include", "video", "rp_video.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert _struct_fields(src, "rp_video_encode_args") == [f[0] for f in video.EncodeArgs._fields_]
    assert video.EncodeArgs._fields_[0][0] == "struct_size"
    assert sorted(set(re.findall(r"\b(rp_video_[a-z_0-9]*)\s*\(", src))) == sorted(video.EXPORTED_SYMBOLS)
    hip = open(os.path.join(vr.ROOT, "robopianist_amd", "csrc", "rp_video.hip")).read()
    for name in video.EXPORTED_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hip), name


def test_missing_library_raises():
    with pytest.raises(video.VideoError, match="not found"):
        video.load_library(os.path.join(vr.ROOT, "no_such_dir", "librp_video.so"))


def test_the_engine_library_does_not_depend_on_the_video_sources():
    """build() keeps rp_video.* out of librp_engine.so's source list, like rp_render.* and rp_audio.*."""
    src = open(os.path.join(vr.ROOT, "__graft_entry__.py")).read()
    listed = re.search(r"own = (.*)\n", src).group(1)
    assert "rp_video." in eval(listed)
    assert "not f.startswith(own)" in src
    for f in ("rp_engine.hip", "rp_task.hip", "rp_render.hip", "rp_audio.hip"):
        assert "rp_video" not in open(os.path.join(vr.ROOT, "robopianist_amd", "csrc", f)).read()


# ---- AVI ---------------------------------------------------------------------------------------------------------------
def _walk(data, start, end):
    """[(fourcc, list kind or None, payload offset, size)] of the chunks in data[start:end]; checks the pad bytes."""
    out, i = [], start
    while i < end:
        fourcc, n = data[i:i + 4], struct.unpack("<I", data[i + 4:i + 8])[0]
        assert i + 8 + n <= end, f"chunk {fourcc} at {i} runs past its parent"
        out.append((fourcc, data[i + 8:i + 12] if fourcc in (b"RIFF", b"LIST") else None, i + 8, n))
        if n & 1:
            assert data[i + 8 + n] == 0, "pad byte"
        i += 8 + n + (n & 1)
    assert i == end
    return out


def _parse_avi(data):
    (riff,) = _walk(data, 0, len(data))
    assert riff[0] == b"RIFF" and riff[1] == b"AVI " and riff[3] == len(data) - 8
    top = _walk(data, 12, len(data))
    assert [(c[0], c[1]) for c in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl = _walk(data, top[0][2] + 4, top[0][2] + top[0][3])
    assert hdrl[0][0] == b"avih" and hdrl[0][3] == 56
    avih = struct.unpack("<14I", data[hdrl[0][2]:hdrl[0][2] + 56])
    streams = []
    for c in hdrl[1:]:
        assert (c[0], c[1]) == (b"LIST", b"strl")
        strh, strf = _walk(data, c[2] + 4, c[2] + c[3])
        assert strh[0] == b"strh" and strh[3] == 56 and strf[0] == b"strf"
        streams.append((data[strh[2]:strh[2] + 56], data[strf[2]:strf[2] + strf[3]]))
    movi_at = top[1][2]          # of the 'movi' fourcc
    movi = _walk(data, movi_at + 4, movi_at + top[1][3])
    index = [struct.unpack("<4sIII", data[top[2][2] + 16 * k:top[2][2] + 16 * k + 16]) for k in range(top[2][3] // 16)]
    assert top[2][3] == 16 * len(movi) and len(index) == len(movi)
    for (fourcc, flags, offset, size), chunk in zip(index, movi):
        assert fourcc == chunk[0] and size == chunk[3] and movi_at + offset == chunk[2] - 8, "idx1 points at the chunk"
        assert flags == 0x10
    return avih, streams, [(c[0], data[c[2]:c[2] + c[3]]) for c in movi]


def _avi_frames():
    cases = [("noise", (30, 44), 90, 0), ("gradient", (30, 44), 90, 0), ("flat", (30, 44), 90, 0),
             ("rendered_like", (30, 44), 90, 0), ("pixel_checkerboard", (30, 44), 90, 0)]
    frames = [vr.case_reference(c)[0] for c in cases]
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames), "odd and even chunk sizes"
    return frames


def test_write_avi_with_sound(tmp_path):
    frames = _avi_frames()
    pcm = np.random.default_rng(5).integers(-32768, 32768, 10007).astype(np.int16)
    n = video.write_avi(tmp_path / "a.avi", frames, (1001, 30000), 30, 44, pcm=pcm, sample_rate=44100)
    data = (tmp_path / "a.avi").read_bytes()
    assert n == len(data)
    avih, streams, movi = _parse_avi(data)
    assert avih[0] == round(1e6 * 1001 / 30000) and avih[4] == len(frames) and avih[6] == 2 and avih[8:10] == (44, 30)
    assert avih[3] & 0x10, "AVIF_HASINDEX"
    (vh, vf), (ah, af) = streams
    assert vh[:8] == b"vidsMJPG"
    scale, rate, start, length = struct.unpack("<4I", vh[20:36])
    assert (scale, rate, start, length) == (1001, 30000, 0, len(frames)), "the frame rate is the exact rational"
    size, w, h, planes, bits, fourcc, image = struct.unpack("<IiiHH4sI", vf[:24])
    assert (size, w, h, planes, bits, fourcc, image) == (40, 44, 30, 1, 24, b"MJPG", 44 * 30 * 3) and len(vf) == 40
    assert ah[:4] == b"auds"
    scale, rate, start, length = struct.unpack("<4I", ah[20:36])
    assert (scale, rate, start, length) == (1, 44100, 0, len(pcm)) and struct.unpack("<I", ah[44:48])[0] == 2
    assert struct.unpack("<HHIIHHH", af) == (1, 1, 44100, 88200, 2, 16, 0), "WAVEFORMATEX: PCM, mono, 16 bit"
    pictures = [p for k, p in movi if k == b"00dc"]
    assert pictures == frames
    for p in pictures:
        assert vr.decode(p).size == (44, 30)
    assert b"".join(p for k, p in movi if k == b"01wb") == pcm.astype("<i2").tobytes()
    # interleaved: a frame, then one frame period of samples; the remainder after the last frame
    kinds = [k for k, _ in movi]
    assert kinds == [b"00dc", b"01wb"] * len(frames) + [b"01wb"]
    per = [len(p) // 2 for k, p in movi if k == b"01wb"]
    edges = [(i + 1) * 44100 * 1001 // 30000 for i in range(len(frames))]
    assert per[:len(frames)] == [b - a for a, b in zip([0] + edges[:-1], edges)] and sum(per) == len(pcm)


def test_write_avi_picture_only_and_short_sound(tmp_path):
    frames = _avi_frames()
    video.write_avi(tmp_path / "v.avi", frames, (1, 20), 30, 44)
    avih, streams, movi = _parse_avi((tmp_path / "v.avi").read_bytes())
    assert avih[6] == 1 and len(streams) == 1 and [k for k, _ in movi] == [b"00dc"] * len(frames)
    assert [p for _, p in movi] == frames and avih[0] == 50000
    # sound shorter than the picture: the later frames have no sound chunk, and none is empty
    pcm = np.arange(3000, dtype=np.int16)
    video.write_avi(tmp_path / "s.avi", frames, (1, 20), 30, 44, pcm=pcm, sample_rate=44100)
    _, _, movi = _parse_avi((tmp_path / "s.avi").read_bytes())
    assert all(len(p) for _, p in movi)
    assert b"".join(p for k, p in movi if k == b"01wb") == pcm.astype("<i2").tobytes()
    with pytest.raises(video.VideoError):
        video.write_avi(tmp_path / "x.avi", [], (1, 20), 30, 44)
    with pytest.raises(video.VideoError):
        video.write_avi(tmp_path / "x.avi", frames, (1, 20), 30, 44, pcm=pcm.astype(np.float32), sample_rate=44100)
    with pytest.raises(video.VideoError):
        video.write_avi(tmp_path / "x.avi", frames, (0, 20), 30, 44)


def test_avi_size_is_arithmetic_and_two_gib_is_refused(tmp_path):
    frames = _avi_frames()
    pcm = np.zeros(4321, np.int16)
    want = video.avi_file_size([len(f) for f in frames], (1, 20), len(pcm), 44100)
    assert video.write_avi(tmp_path / "a.avi", frames, (1, 20), 30, 44, pcm=pcm, sample_rate=44100) == want
    assert video.avi_file_size([len(f) for f in frames], (1, 20)) == video.write_avi(tmp_path / "b.avi", frames, (1, 20), 30, 44)
    # 4096 frames of 512 KiB are 2 GiB of payload alone: refused from the lengths, nothing is written
    with pytest.raises(video.VideoError, match="2 GiB"):
        video.avi_file_size([512 * 1024] * 4096, (1, 20))
    assert video.avi_file_size([512 * 1024] * 4000, (1, 20)) < video.AVI_MAX_BYTES
    below = video.avi_file_size([1000] * 10, (1, 20))
    fill = video.AVI_MAX_BYTES - below
    # (chunks are padded to even sizes, so a file's size is even: 2 GiB - 2 is the largest there is)
    assert fill & 1 and video.avi_file_size([1000] * 9 + [1000 + fill - 1], (1, 20)) == video.AVI_MAX_BYTES - 1
    with pytest.raises(video.VideoError, match="2 GiB"):
        video.avi_file_size([1000] * 9 + [1000 + fill], (1, 20))


# ---- the sanitizers, in a program of its own ---------------------------------------------------------------------------
def test_host_routines_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The extreme cases (noise, the checkerboard of blocks and a flat image at qualities 100 and 1; one block, padding,
    segments of two and three chunks) through rpv_encode_host in a stand-alone program, every output buffer exactly as
    long as the file.  Nothing sanitised is loaded into this process."""
    exe, log = vr.build_sanitizer_program(str(tmp_path))
    if exe is None:
        pytest.skip("this g++ cannot link -fsanitize=address,undefined: " + log.strip().splitlines()[-1])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "FAILED" not in r.stdout and "runtime error" not in r.stderr
