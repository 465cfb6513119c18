"""PCM16 WAV output, as ``soundfile.write(path, wav, 16000)`` does by default (InferAPI.py:98).

libsndfile's normalised float->short conversion rounds ``x * 32767`` to nearest
(lrintf, ties to even) and clips; soundfile is not installed offline, so the
writer is restated here (parity of the bytes is unpinned, the float waveform is
the parity target).
"""
from __future__ import annotations

import struct

import numpy as np


def pcm16(wav, scale: float = 32767.0) -> np.ndarray:
    x = np.asarray(wav, dtype=np.float32).reshape(-1) * np.float32(scale)
    return np.clip(np.rint(x), -32768, 32767).astype("<i2")


def write_pcm16(path: str, wav, sample_rate: int = 16000, scale: float = 32767.0) -> None:
    """``scale`` 32768.0 inverts ``read_wav`` (x / 32768) exactly, so samples read from a file and written back keep
    their bits (with 32767 an untouched sample of |x| >= 0.5 comes back one step off); the default is libsndfile's."""
    data = pcm16(wav, scale).tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, sample_rate, sample_rate * 2, 2, 16))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def read_pcm16(path: str):
    with open(path, "rb") as f:
        raw = f.read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
    sr = struct.unpack("<I", raw[24:28])[0]
    n = struct.unpack("<I", raw[40:44])[0]
    return np.frombuffer(raw[44:44 + n], dtype="<i2"), sr


def read_wav(path: str):
    """Mono PCM16 WAV -> (float32 samples in [-1, 1] (x / 32768), sample rate).  Walks the RIFF chunks (a file may
    carry LIST or other chunks before ``data``); anything but mono 16-bit PCM raises ValueError."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt = data = None
    pos = 12
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
        body = raw[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = body
        elif cid == b"data":
            data = body
            break
        pos += 8 + size + (size & 1)  # chunks are word aligned
    if fmt is None or len(fmt) < 16 or data is None:
        raise ValueError(f"{path}: missing fmt or data chunk")
    tag, channels, sr, _, _, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag != 1 or channels != 1 or bits != 16:
        raise ValueError(f"{path}: only mono PCM16 is read (format {tag}, {channels} channels, {bits} bits)")
    x = np.frombuffer(data[:len(data) // 2 * 2], dtype="<i2").astype(np.float32) / np.float32(32768.0)
    return x, sr


def read_audio(path: str):
    """WAV -> (float32 (N, channels) in [-1, 1], sample rate): 16- or 24-bit PCM (x / 32768, x / 8388608) or 32-bit
    IEEE float, 1 to 8 channels, a plain ``fmt `` chunk or WAVE_FORMAT_EXTENSIBLE (the format is the sub-format's first
    two bytes).  The same chunk walk as ``read_wav``; a mono PCM16 file gives ``read_wav``'s floats.  Anything else
    raises ValueError."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt = data = None
    pos = 12
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
        body = raw[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = body
        elif cid == b"data":
            data = body
            break
        pos += 8 + size + (size & 1)  # chunks are word aligned
    if fmt is None or len(fmt) < 16 or data is None:
        raise ValueError(f"{path}: missing fmt or data chunk")
    tag, channels, sr, _, _, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE:  # WAVE_FORMAT_EXTENSIBLE: cbSize, valid bits, channel mask, then the sub-format GUID
        if len(fmt) < 26:
            raise ValueError(f"{path}: truncated WAVE_FORMAT_EXTENSIBLE fmt chunk")
        tag = struct.unpack("<H", fmt[24:26])[0]
    if not 1 <= channels <= 8:
        raise ValueError(f"{path}: {channels} channels, 1 to 8 are read")
    if (tag, bits) not in ((1, 16), (1, 24), (3, 32)):
        raise ValueError(f"{path}: only 16- and 24-bit PCM and 32-bit float are read (format {tag}, {bits} bits)")
    frame = channels * bits // 8
    data = data[:len(data) // frame * frame]
    if bits == 16:
        x = np.frombuffer(data, dtype="<i2").astype(np.float32) / np.float32(32768.0)
    elif bits == 24:
        b = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) / np.float32(8388608.0)
    else:
        x = np.frombuffer(data, dtype="<f4").astype(np.float32)
    return x.reshape(-1, channels), sr
