"""Audio files.  The reference plays through PyAudio and writes its recording with the stdlib `wave` module
(robopianist/music/audio.py, wrappers/sound.py:72-78); playback needs a sound device and is left out, the file
writer is here."""

from __future__ import annotations

import wave
from pathlib import Path
from typing import Union

import numpy as np

from robopianist_amd.music import constants as consts


def write_wav(path: Union[str, Path], pcm: np.ndarray, sample_rate: int = consts.SAMPLING_RATE) -> None:
    """Writes int16 samples as a mono 16-bit WAV file."""
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise ValueError(f"write_wav expects a one-dimensional int16 array, got {pcm.dtype} {pcm.shape}")
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(int(sample_rate))
        wf.writeframes(pcm.astype("<i2").tobytes())
