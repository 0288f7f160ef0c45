"""What every environment hears, per step: ctypes binding of include/audio/rp_hear.h (librp_hear.so).

The synthesiser (music/synthesizer.py) turns a finished episode into a sound file.  `Hearing` serves a policy while it
plays: `track` consumes the key trace of one control step of every env into a voice bank (per key the two newest
notes), `spectrum` synthesises the last `window` samples of that bank and analyses them into one magnitude per bin.
Everything stays on the device.  The sound is the synthesiser's (its timbre table and note rule); the analysis is the
table of `make_analysis`: data that is packed into the create blob, not code.  Like the synthesiser there is no CPU
fallback: a missing library is an error.
"""

from __future__ import annotations

import ctypes
import math
import struct
from typing import Optional, Tuple

import numpy as np

from robopianist_amd import _abi
from robopianist_amd.music import constants as consts
from robopianist_amd.music import synthesizer

EXPORTED_SYMBOLS = ("rp_hear_create", "rp_hear_destroy", "rp_hear_track", "rp_hear_spectrum", "rp_hear_dim",
                    "rp_hear_last_error")

N_KEYS = consts.NUM_KEYS
N_SLOTS = 2              # notes kept per key: the newest and the one before
N_STATE = 8              # state words per env (rp_hear.h)
MIN_WINDOW, MAX_WINDOW, MAX_BINS = 64, 4096, 128
_BLOB_MAGIC, _BLOB_VERSION = 0x41485052, 1


class HearingError(RuntimeError):
    pass


# ------------------------------------------------------------------------------------------------------- analysis
def key_frequencies() -> np.ndarray:
    """The 88 key fundamentals, Hz."""
    p = np.arange(N_KEYS) + consts.MIN_MIDI_PITCH_PIANO
    return 440.0 * 2.0 ** ((p - 69) / 12.0)


def make_analysis(sample_rate: float, window: int, freqs=None, cycles: float = 16.0) -> Tuple[np.ndarray, np.ndarray]:
    """(C, S) float32 [window][B]: bin b is a Hann-windowed complex tone at freqs[b] over the newest
    L_b = min(window, ceil(cycles sr / f_b)) samples of the window, normalised so that a unit sine at f_b reads 1.
    With i = j - (window - L_b): for i >= 0, h_i = 0.5 - 0.5 cos(2 pi (i + 0.5) / L_b), w_i = 2 h_i / sum h,
    C = w_i cos(2 pi frac(f_b i / sr)), S = w_i sin(2 pi frac(f_b i / sr)); elsewhere both are 0.  Computed in float64 and
    rounded.  `freqs` defaults to the 88 key fundamentals."""
    W, sr = int(window), float(sample_rate)
    f = key_frequencies() if freqs is None else np.asarray(freqs, np.float64).reshape(-1)
    C = np.zeros((W, len(f)), np.float64)
    S = np.zeros((W, len(f)), np.float64)
    for b, fb in enumerate(f):
        L = min(W, int(math.ceil(float(cycles) * sr / fb)))
        i = np.arange(L, dtype=np.float64)
        h = 0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 0.5) / L)
        w = 2.0 * h / h.sum()
        x = fb * i / sr
        ph = 2.0 * np.pi * (x - np.floor(x))
        C[W - L:, b] = w * np.cos(ph)
        S[W - L:, b] = w * np.sin(ph)
    return C.astype(np.float32), S.astype(np.float32)


def make_analysis_blob(C: np.ndarray, S: np.ndarray) -> bytes:
    """The analysis blob of rp_hear_create: u32 magic, u32 version, i32 W, i32 B, then float32 C[W][B], S[W][B]."""
    C, S = np.asarray(C), np.asarray(S)
    if C.ndim != 2 or C.shape != S.shape:
        raise ValueError(f"C and S must be two tables of one shape [W][B], got {C.shape} and {S.shape}")
    W, B = C.shape
    if not (MIN_WINDOW <= W <= MAX_WINDOW and W % 64 == 0):
        raise ValueError(f"the window must be a multiple of 64 in {MIN_WINDOW}..{MAX_WINDOW}, got {W}")
    if not 1 <= B <= MAX_BINS:
        raise ValueError(f"the number of bins must be in 1..{MAX_BINS}, got {B}")
    return (struct.pack("<IIii", _BLOB_MAGIC, _BLOB_VERSION, W, B)
            + np.ascontiguousarray(C, "<f4").tobytes() + np.ascontiguousarray(S, "<f4").tobytes())


# ------------------------------------------------------------------------------------------------------- binding
class Bank(ctypes.Structure):
    """rp_hear_bank (include/audio/rp_hear.h)."""
    _fields_ = [
        ("t_on", ctypes.c_void_p),
        ("t_off", ctypes.c_void_p),
        ("state", ctypes.c_void_p),
    ]


class TrackArgs(ctypes.Structure):
    """rp_hear_track_args."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("trace", ctypes.c_void_p),
        ("n_sub", ctypes.c_int),
        ("pedal", ctypes.c_void_p),
        ("restart", ctypes.c_void_p),
        ("dt", ctypes.c_double),
        ("bank", Bank),
        ("env_first", ctypes.c_int), ("env_count", ctypes.c_int),
        ("hip_stream", ctypes.c_void_p),
    ]


class SpectrumArgs(ctypes.Structure):
    """rp_hear_spectrum_args."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("bank", Bank),
        ("dt", ctypes.c_double),
        ("env_first", ctypes.c_int), ("env_count", ctypes.c_int),
        ("window", ctypes.c_void_p),
        ("spectrum", ctypes.c_void_p),
        ("hip_stream", ctypes.c_void_p),
    ]


_table = _abi.HandleTable("rp_hear_", {"track": TrackArgs, "spectrum": SpectrumArgs}, HearingError, "RP_HEAR_LIB",
                          "librp_hear.so", "hearing",
                          create=[ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int])
LIB_PATH = _table.path
load_library, declare = _table.load, _table.declare


class Hearing(_abi.Owner):
    """Batched audio observation.  `analysis` is a (C, S) pair of `make_analysis` (default: the 88 key fundamentals at
    `sample_rate` over `window` samples); `timbre` defaults to the synthesiser's.  The voice bank lives in device tensors
    of this object: `t_on`, `t_off` float64 [E, 88, 2] and `state` int32 [E, 8] (rp_hear.h); a new object's bank is empty."""

    def __init__(self, n_envs: int, sample_rate: int = 16000, window: int = 2048, analysis=None,
                 timbre: Optional[dict] = None, physics_timestep: float = 0.005, max_substeps_per_call: int = 64,
                 device_id: int = 0):
        import torch
        self.n_envs, self.sample_rate, self.device_id = int(n_envs), sample_rate, int(device_id)
        self.physics_timestep = float(physics_timestep)
        self.max_substeps_per_call = int(max_substeps_per_call)
        self.timbre = synthesizer.DEFAULT_TIMBRE if timbre is None else timbre
        self.analysis = make_analysis(sample_rate, window) if analysis is None else analysis
        self.audio_blob = synthesizer.make_audio_blob(self.timbre, sample_rate)
        self.analysis_blob = make_analysis_blob(*self.analysis)
        self.window, self.n_bins = (int(n) for n in np.asarray(self.analysis[0]).shape)
        self._handle = _abi.Handle(_table, self.audio_blob, len(self.audio_blob), self.analysis_blob, len(self.analysis_blob),
                                   self.n_envs, self.max_substeps_per_call, self.device_id)
        dev = self.device = torch.device("cuda", self.device_id)
        E = self.n_envs
        self.t_on = torch.full((E, N_KEYS, N_SLOTS), -1.0, dtype=torch.float64, device=dev)
        self.t_off = torch.full((E, N_KEYS, N_SLOTS), -1.0, dtype=torch.float64, device=dev)
        self.state = torch.zeros((E, N_STATE), dtype=torch.int32, device=dev)
        self._out = None

    # -- helpers ---------------------------------------------------------------------------------------------
    @property
    def forgotten(self):
        """[n_envs] int32 device view: the voices that were pushed out of the bank while they still sounded."""
        return self.state[:, 7]

    @property
    def substeps(self):
        """[n_envs] int32 device view: the substeps consumed since the env's restart."""
        return self.state[:, 6]

    def outputs(self):
        """(spectrum float32 [E, B], window float32 [E, W]): this object's cached buffers."""
        import torch
        if self._out is None:
            self._out = (torch.zeros((self.n_envs, self.n_bins), dtype=torch.float32, device=self.device),
                         torch.zeros((self.n_envs, self.window), dtype=torch.float32, device=self.device))
        return self._out

    def _stream(self, hip_stream):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream if hip_stream is None else hip_stream

    def _bank(self) -> Bank:
        return Bank(self.t_on.data_ptr(), self.t_off.data_ptr(), self.state.data_ptr())

    def _env_window(self, env_first, env_count):
        return int(env_first), int(self.n_envs - env_first if env_count is None else env_count)

    def _flags(self, x, name):
        """[E] int32 device tensor of a per-env flag given as a device tensor of any integer / bool type."""
        import torch
        if x is None:
            return None
        if not isinstance(x, torch.Tensor) or not x.is_cuda or tuple(x.shape) != (self.n_envs,):
            raise HearingError(f"{name}: expected a device tensor of {self.n_envs} flags")
        return x.to(torch.int32).contiguous()

    # -- the two calls -----------------------------------------------------------------------------------------
    def track_args(self, trace, pedal=None, restart=None, dt=None, env_first=0, env_count=None, hip_stream=None) -> TrackArgs:
        first, count = self._env_window(env_first, env_count)
        return _abi.fill(TrackArgs, trace=trace.data_ptr(), n_sub=int(trace.shape[1]),
                         pedal=None if pedal is None else pedal.data_ptr(),
                         restart=None if restart is None else restart.data_ptr(),
                         dt=float(self.physics_timestep if dt is None else dt), bank=self._bank(), env_first=first,
                         env_count=count, hip_stream=self._stream(hip_stream))

    def spectrum_args(self, spectrum, window=None, dt=None, env_first=0, env_count=None, hip_stream=None) -> SpectrumArgs:
        first, count = self._env_window(env_first, env_count)
        return _abi.fill(SpectrumArgs, bank=self._bank(), dt=float(self.physics_timestep if dt is None else dt),
                         env_first=first, env_count=count, window=None if window is None else window.data_ptr(),
                         spectrum=None if spectrum is None else spectrum.data_ptr(), hip_stream=self._stream(hip_stream))

    def track_raw(self, args: TrackArgs) -> int:
        """rp_hear_track with a caller-made argument block; returns the C return code."""
        return self._handle.call_raw("track", args)

    def spectrum_raw(self, args: SpectrumArgs) -> int:
        """rp_hear_spectrum with a caller-made argument block; returns the C return code."""
        return self._handle.call_raw("spectrum", args)

    def _check_trace(self, trace):
        import torch
        if (not isinstance(trace, torch.Tensor) or not trace.is_cuda or trace.dim() != 3 or trace.shape[0] != self.n_envs
                or trace.shape[2] != 4 or trace.element_size() != 4 or trace.is_floating_point() or not trace.is_contiguous()):
            raise HearingError(f"trace: expected a contiguous 32-bit integer device tensor [{self.n_envs}, n_sub, 4]")

    def track(self, trace, pedal=None, restart=None, env_first=0, env_count=None, dt=None, hip_stream=None) -> None:
        """Consumes `trace` [E, n_sub, 4] (Environment.key_trace of one control step) into the bank of the envs of the
        window.  `pedal` [E]: nonzero holds the sustain pedal down in every row of this call (in addition to bit 88 of
        the rows); `restart` [E]: nonzero empties the env's bank instead (its rows are not consumed).  Both are device
        tensors of any integer or bool type, or None."""
        self._check_trace(trace)
        pedal, restart = self._flags(pedal, "pedal"), self._flags(restart, "restart")   # (kept alive until the launch)
        self._handle.call("track", self.track_args(trace, pedal, restart, dt, env_first, env_count, hip_stream))

    def spectrum(self, window=False, env_first=0, env_count=None, dt=None, hip_stream=None):
        """The magnitudes [E, B] of the newest `window` samples of what the bank sounds like, or (magnitudes, samples
        [E, W]) with `window=True`.  The tensors are this object's cached buffers and are overwritten by the next
        call; envs outside the window keep their rows."""
        spec, wave = self.outputs()
        self._handle.call("spectrum", self.spectrum_args(spec, wave if window else None, dt, env_first, env_count, hip_stream))
        return (spec, wave) if window else spec

    def observe(self, trace, pedal=None, restart=None, window=False, env_first=0, env_count=None, dt=None, hip_stream=None):
        """`track`, then `spectrum`."""
        self.track(trace, pedal, restart, env_first, env_count, dt, hip_stream)
        return self.spectrum(window, env_first, env_count, dt, hip_stream)

    # -- checkpoint ----------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"t_on": self.t_on.detach().clone(), "t_off": self.t_off.detach().clone(), "state": self.state.detach().clone()}

    def load_state_dict(self, sd):
        for name in ("t_on", "t_off", "state"):
            getattr(self, name).copy_(sd[name].to(self.device))
