"""ctypes binding of the JPEG encoder's C ABI (include/video/rp_video.h, librp_video.so) and the AVI writer.

`Encoder` turns a batch of rendered frames (uint8 [N,H,W,3] on the device, what `Renderer.render` returns) into one
baseline JPEG file per frame, on the caller's HIP stream, into torch tensors it caches per row size.  Like the engine,
it has no CPU fallback: a missing library is an error.

`write_avi` is pure Python: it puts such frames, and optionally 16-bit mono PCM, into a RIFF AVI file (Motion-JPEG
video stream, PCM audio stream, `idx1` index).
"""

from __future__ import annotations

import ctypes
import struct
from pathlib import Path
from typing import Optional, Sequence, Tuple, Union

import numpy as np

from robopianist_amd import _abi

EXPORTED_SYMBOLS = ("rp_video_create", "rp_video_destroy", "rp_video_encode", "rp_video_max_bytes", "rp_video_header",
                    "rp_video_dim", "rp_video_last_error")


class VideoError(RuntimeError):
    pass


class EncodeArgs(ctypes.Structure):
    """rp_video_encode_args (include/video/rp_video.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("rgb", ctypes.c_void_p),
        ("frame_first", ctypes.c_int), ("frame_count", ctypes.c_int),
        ("bytes_cap", ctypes.c_int),
        ("bytes", ctypes.c_void_p),
        ("length", ctypes.c_void_p),
        ("hip_stream", ctypes.c_void_p),
    ]


def make_args(frame_first, frame_count, bytes_cap, rgb=None, out_bytes=None, length=None, hip_stream=None) -> EncodeArgs:
    """Fills an rp_video_encode_args; the array arguments are raw addresses (or None)."""
    return _abi.fill(EncodeArgs, rgb=rgb, bytes=out_bytes, length=length, frame_first=int(frame_first),
                     frame_count=int(frame_count), bytes_cap=int(bytes_cap), hip_stream=hip_stream)


_table = _abi.HandleTable("rp_video_", {"encode": EncodeArgs}, VideoError, "RP_VIDEO_LIB", "librp_video.so", "video",
                          create=[ctypes.c_int] * 5,
                          extra={"max_bytes": [], "header": [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]})
LIB_PATH = _table.path
load_library, declare = _table.load, _table.declare


def read_header(L, handle, prefix: str = "rp_video_") -> bytes:
    """The constant header bytes of an encoder (rp_video_header)."""
    n = ctypes.c_int(0)
    if getattr(L, prefix + "header")(handle, None, ctypes.byref(n)) != 0:
        raise VideoError(getattr(L, prefix + "last_error")().decode())
    buf = (ctypes.c_ubyte * n.value)()
    getattr(L, prefix + "header")(handle, buf, ctypes.byref(n))
    return bytes(buf)


class Encoder(_abi.Owner):
    """Batched JPEG encoder of `max_frames` frames of one size and quality."""

    def __init__(self, height: int, width: int, max_frames: int, quality: int = 90, device_id: int = 0):
        self.height, self.width, self.max_frames = int(height), int(width), int(max_frames)
        self.quality, self.device_id = int(quality), int(device_id)
        self._handle = _abi.Handle(_table, self.height, self.width, self.max_frames, self.quality, self.device_id)
        self.max_bytes = self._L.rp_video_max_bytes(self._h)   # a frame never needs more: the default row size
        self.header = read_header(self._L, self._h)
        self._out = {}

    def outputs(self, bytes_cap: Optional[int] = None):
        """The cached output tensors of this row size: (bytes uint8 [N,bytes_cap], length int32 [N]), allocated at
        the first call."""
        import torch
        cap = self.max_bytes if bytes_cap is None else int(bytes_cap)
        if cap not in self._out:
            dev = torch.device("cuda", self.device_id)
            self._out[cap] = (torch.zeros((self.max_frames, max(cap, 0)), dtype=torch.uint8, device=dev),
                              torch.zeros((self.max_frames,), dtype=torch.int32, device=dev))
        return self._out[cap]

    def encode_raw(self, args: EncodeArgs) -> int:
        """rp_video_encode with a caller-made argument block; returns the C return code (see last_error())."""
        return self._handle.call_raw("encode", args)

    def encode(self, rgb, frame_first: int = 0, frame_count: Optional[int] = None, bytes_cap: Optional[int] = None,
               hip_stream=None):
        """rgb: contiguous uint8 device tensor [max_frames,H,W,3].  Returns (bytes, length): the cached device tensors
        of this row size; row f holds frame f's JPEG file in its first length[f] bytes, and length[f] = -(bytes needed)
        if it did not fit `bytes_cap` (default: `max_bytes`, which always fits).  Rows outside the window keep what
        they held.  Enqueues on `hip_stream` (default: torch's current stream)."""
        import torch
        shape = (self.max_frames, self.height, self.width, 3)
        if tuple(rgb.shape) != shape or rgb.dtype != torch.uint8 or not rgb.is_contiguous() or not rgb.is_cuda:
            raise VideoError(f"encode: expected a contiguous uint8 device tensor of shape {shape}, got "
                             f"{rgb.dtype} {tuple(rgb.shape)}")
        if hip_stream is None:
            hip_stream = torch.cuda.current_stream(torch.device("cuda", self.device_id)).cuda_stream
        out, length = self.outputs(bytes_cap)
        self._handle.call("encode", make_args(
            frame_first, self.max_frames - frame_first if frame_count is None else frame_count, out.shape[1],
            rgb=rgb.data_ptr(), out_bytes=out.data_ptr(), length=length.data_ptr(), hip_stream=hip_stream))
        return out, length

    def frames(self, rgb, frame_first: int = 0, frame_count: Optional[int] = None, bytes_cap: Optional[int] = None):
        """encode(), then the window's files as a list of `bytes` on the host (one read-back of the lengths, then one
        copy per frame of exactly its bytes)."""
        out, length = self.encode(rgb, frame_first, frame_count, bytes_cap)
        count = self.max_frames - frame_first if frame_count is None else frame_count
        lengths = length[frame_first:frame_first + count].cpu().tolist()
        files = []
        for i, n in enumerate(lengths):
            if n < 0:
                raise VideoError(f"frame {frame_first + i} needs {-n} bytes, bytes_cap is {out.shape[1]}")
            files.append(out[frame_first + i, :n].cpu().numpy().tobytes())
        return files


# ---- AVI --------------------------------------------------------------------------------------------------------------
AVI_MAX_BYTES = 2 ** 31 - 1      # plain AVI (one RIFF chunk, no OpenDML extension)
_AVIF_HASINDEX, _AVIF_ISINTERLEAVED, _AVIIF_KEYFRAME = 0x10, 0x100, 0x10


def _chunk(fourcc: bytes, data: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def _list(kind: bytes, body: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body


def audio_split(n_frames: int, n_samples: int, frame_period: Tuple[int, int], sample_rate: int):
    """Samples written after each frame: frame i is followed by the samples up to floor((i + 1) sample_rate num / den),
    and the last entry (index n_frames) is the remainder."""
    num, den = frame_period
    edges = [min(n_samples, ((i + 1) * sample_rate * num) // den) for i in range(n_frames)]
    counts = [b - a for a, b in zip([0] + edges[:-1], edges)]
    return counts + [n_samples - (edges[-1] if edges else 0)]


def _hdrl(n_frames, frame_period, height, width, max_frame, n_samples, sample_rate) -> bytes:
    num, den = frame_period
    has_audio = n_samples is not None
    usec = (1000000 * num + den // 2) // den
    rate = (max_frame * den + num - 1) // num + (2 * sample_rate if has_audio else 0)
    avih = struct.pack("<14I", usec, min(rate, 0xFFFFFFFF), 0, _AVIF_HASINDEX | (_AVIF_ISINTERLEAVED if has_audio else 0),
                       n_frames, 0, 2 if has_audio else 1, max_frame, width, height, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, num, den, 0, n_frames, max_frame, 0xFFFFFFFF, 0,
                                           0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    body = _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf))
    if has_audio:
        strh = b"auds" + b"\0\0\0\0" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, sample_rate, 0, n_samples,
                                                   2 * sample_rate, 0xFFFFFFFF, 2, 0, 0, 0, 0)
        strf = struct.pack("<HHIIHHH", 1, 1, sample_rate, 2 * sample_rate, 2, 16, 0)   # WAVEFORMATEX, PCM
        body += _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf))
    return _list(b"hdrl", body)


def avi_file_size(frame_lengths: Sequence[int], frame_period: Tuple[int, int], n_samples: Optional[int] = None,
                  sample_rate: Optional[int] = None) -> int:
    """The size of the file write_avi would write, from the frames' lengths alone; raises VideoError beyond
    AVI_MAX_BYTES."""
    payloads = [int(n) for n in frame_lengths]
    if n_samples is not None:
        payloads += [2 * c for c in audio_split(len(frame_lengths), n_samples, frame_period, sample_rate) if c]
    movi = 4 + sum(8 + n + (n & 1) for n in payloads)
    hdrl = len(_hdrl(len(frame_lengths), frame_period, 1, 1, 0, n_samples, sample_rate or 0))
    total = 12 + hdrl + 8 + movi + 8 + 16 * len(payloads)
    if total > AVI_MAX_BYTES:
        raise VideoError(f"the AVI file would be {total} bytes; a plain AVI holds at most 2 GiB - 1 "
                         "(write fewer or smaller frames per file)")
    return total


def write_avi(path: Union[str, Path], frames: Sequence[bytes], frame_period: Tuple[int, int], height: int, width: int,
              pcm=None, sample_rate: Optional[int] = None) -> int:
    """Writes JPEG files `frames` as the Motion-JPEG stream of an AVI file, one every frame_period = (num, den)
    seconds (kept exactly: dwScale = num, dwRate = den), with int16 mono `pcm` at `sample_rate` as a second stream.
    The audio is interleaved: one frame period of samples after each frame, the remainder after the last.  Returns the
    file's size."""
    num, den = int(frame_period[0]), int(frame_period[1])
    if num < 1 or den < 1 or max(num, den) > 0xFFFFFFFF:
        raise VideoError(f"frame_period must be a pair of positive 32-bit integers, got {frame_period}")
    if not frames:
        raise VideoError("write_avi needs at least one frame")
    frames = [bytes(f) for f in frames]
    n_samples = None
    if pcm is not None:
        pcm = np.asarray(pcm)
        if pcm.dtype != np.int16 or pcm.ndim != 1:
            raise VideoError(f"write_avi expects a one-dimensional int16 array, got {pcm.dtype} {pcm.shape}")
        if sample_rate is None or int(sample_rate) < 1:
            raise VideoError("write_avi needs the sample_rate of pcm")
        sample_rate, n_samples = int(sample_rate), len(pcm)
        raw = pcm.astype("<i2").tobytes()
    total = avi_file_size([len(f) for f in frames], (num, den), n_samples, sample_rate)
    chunks = []
    if pcm is None:
        chunks = [(b"00dc", f) for f in frames]
    else:
        at = 0
        counts = audio_split(len(frames), n_samples, (num, den), sample_rate)
        for f, c in zip(frames, counts):
            chunks.append((b"00dc", f))
            if c:
                chunks.append((b"01wb", raw[2 * at:2 * (at + c)]))
            at += c
        if counts[-1]:
            chunks.append((b"01wb", raw[2 * at:]))
    movi, index = [b"movi"], []
    offset = 4          # of the next chunk, from the 'movi' fourcc
    for fourcc, data in chunks:
        piece = _chunk(fourcc, data)
        index.append(struct.pack("<4sIII", fourcc, _AVIIF_KEYFRAME, offset, len(data)))
        movi.append(piece)
        offset += len(piece)
    hdrl = _hdrl(len(frames), (num, den), int(height), int(width), max(len(f) for f in frames), n_samples, sample_rate or 0)
    body = b"AVI " + hdrl + b"LIST" + struct.pack("<I", offset) + b"".join(movi) + _chunk(b"idx1", b"".join(index))
    data = b"RIFF" + struct.pack("<I", len(body)) + body
    assert len(data) == total
    with open(path, "wb") as fh:
        fh.write(data)
    return total
