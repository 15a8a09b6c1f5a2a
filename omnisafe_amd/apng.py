"""Truecolour 8-bit PNG and animated PNG (APNG) files with the standard library only (``zlib``, ``struct``): the replays
of :meth:`omnisafe_amd.evaluator.Evaluator.render` must be writable where no imaging package is installed.

    write_png(path, frame)              frame: (H, W, 3) uint8
    write_apng(path, frames, fps)       frames: (H, W, 3) arrays, (n, H, W, 3) chunks, or an iterator of either
    read_apng(path) -> [(H, W, 3), ...]  the files written here (a plain PNG reads as one frame)

Every scanline uses filter type 0; every frame of an animation covers the whole canvas and replaces it (dispose 0,
blend 0) and is shown for 1 / fps seconds; the animation loops for ever.  The first frame is the default image
(``fcTL`` before ``IDAT``), so a viewer without APNG support shows frame 0.  ``frames`` is consumed as it comes: a long
replay never sits in host memory at once; the frame count in ``acTL`` is filled in at the end.
"""
from __future__ import annotations

import struct
import zlib
from fractions import Fraction

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def _scanlines(frame: np.ndarray, level: int) -> bytes:
    """The zlib stream of a frame: a filter byte 0 in front of every row."""
    h, w, _ = frame.shape
    rows = np.zeros((h, 1 + 3 * w), np.uint8)
    rows[:, 1:] = frame.reshape(h, 3 * w)
    return zlib.compress(rows.tobytes(), level)


def _frames(frames):
    """Single (H, W, 3) frames out of frames, (n, H, W, 3) chunks or an iterable of either."""
    if isinstance(frames, np.ndarray):
        frames = [frames]
    for item in frames:
        item = np.asarray(item)
        if item.dtype != np.uint8 or item.ndim not in (3, 4) or item.shape[-1] != 3:
            raise ValueError(f'frames are (H, W, 3) uint8 arrays or (n, H, W, 3) chunks, not {item.dtype}{item.shape}')
        yield from (item if item.ndim == 4 else item[None])


def _ihdr(w: int, h: int) -> bytes:
    return _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))  # 8 bits, colour type 2 (RGB)


def write_png(path, frame, level: int = 6) -> None:
    frame = next(_frames(frame))
    h, w, _ = frame.shape
    with open(path, 'wb') as f:
        f.write(SIGNATURE + _ihdr(w, h) + _chunk(b'IDAT', _scanlines(frame, level)) + _chunk(b'IEND', b''))


def write_apng(path, frames, fps=30, level: int = 6) -> int:
    """Returns the number of frames written (at least one is required)."""
    delay = 1 / Fraction(fps).limit_denominator(1000)
    delay = delay.limit_denominator(65535)
    seq = n = 0
    shape = None
    with open(path, 'wb') as f:
        for frame in _frames(frames):
            if shape is None:
                shape = frame.shape
                h, w, _ = shape
                f.write(SIGNATURE + _ihdr(w, h))
                actl_at = f.tell()
                f.write(_chunk(b'acTL', struct.pack('>II', 0, 0)))
            elif frame.shape != shape:
                raise ValueError(f'frame {n} is {frame.shape}, the animation {shape}')
            f.write(_chunk(b'fcTL', struct.pack('>IIIIIHHBB', seq, w, h, 0, 0, delay.numerator, delay.denominator,
                                                0, 0)))
            seq += 1
            data = _scanlines(frame, level)
            if n == 0:
                f.write(_chunk(b'IDAT', data))
            else:
                f.write(_chunk(b'fdAT', struct.pack('>I', seq) + data))
                seq += 1
            n += 1
        if n == 0:
            raise ValueError('an animation needs at least one frame')
        f.write(_chunk(b'IEND', b''))
        f.seek(actl_at)
        f.write(_chunk(b'acTL', struct.pack('>II', n, 0)))  # num_frames, num_plays 0: for ever
    return n


def chunks(path):
    """(type, data) of every chunk of a PNG file, CRCs checked."""
    with open(path, 'rb') as f:
        raw = f.read()
    if raw[:8] != SIGNATURE:
        raise ValueError(f'{path}: not a PNG file')
    at, out = 8, []
    while at < len(raw):
        (size,) = struct.unpack('>I', raw[at:at + 4])
        kind, data = raw[at + 4:at + 8], raw[at + 8:at + 8 + size]
        (crc,) = struct.unpack('>I', raw[at + 8 + size:at + 12 + size])
        if crc != zlib.crc32(kind + data) & 0xFFFFFFFF:
            raise ValueError(f'{path}: bad CRC in {kind!r}')
        out.append((kind, data))
        at += 12 + size
    return out


def read_apng(path) -> list:
    """The frames of a file written by this module, each (H, W, 3) uint8."""
    w = h = None
    streams: list[bytes] = []
    for kind, data in chunks(path):
        if kind == b'IHDR':
            w, h, depth, colour, _, _, interlace = struct.unpack('>IIBBBBB', data)
            if (depth, colour, interlace) != (8, 2, 0):
                raise ValueError(f'{path}: only 8-bit truecolour without interlace is read here')
        elif kind == b'fcTL':
            if struct.unpack('>IIII', data[4:20]) != (w, h, 0, 0):
                raise ValueError(f'{path}: only whole-canvas frames are read here')
            streams.append(b'')
        elif kind in (b'IDAT', b'fdAT'):
            if not streams:  # a plain PNG: no fcTL in front of IDAT
                streams.append(b'')
            streams[-1] += data if kind == b'IDAT' else data[4:]
    out = []
    for s in streams:
        rows = np.frombuffer(zlib.decompress(s), np.uint8).reshape(h, 1 + 3 * w)
        if rows[:, 0].any():
            raise ValueError(f'{path}: only filter type 0 is read here')
        out.append(rows[:, 1:].reshape(h, w, 3).copy())
    return out


__all__ = ['write_png', 'write_apng', 'read_apng']
