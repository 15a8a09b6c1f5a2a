"""Host side of osa_render_episode (csrc/render_kernels.hip): frames of the top-down picture that
include/omnisafe_amd.h specifies, rasterised on the device from the state rows of a trace or of a live env -- and of
osa_custom_render_episode (csrc/scene_render.h), the same for a class of ``register_device_env`` whose description has
a ``draw()``: name it with a :class:`CustomScene` wherever an ``env_kind`` is taken.

``rasterise`` is one launch into a device tensor; ``stream_frames`` renders an episode in chunks of bounded device
memory and hands each chunk to the host through one pinned buffer, as numpy views that are valid until the next chunk.
There is no host rasteriser: without the library or a GPU this raises (omnisafe_amd._lib).
"""
from __future__ import annotations

import time
from typing import NamedTuple

import torch

from . import _lib

CAMERAS = {'fixed': 0, 'track': 1}
CHUNK_BYTES = 32 << 20  # device (and pinned host) bytes of a chunk of frames


class CustomScene(NamedTuple):
    """In the place of an ``env_kind``: a class of ``register_device_env`` that draws (``cls.draws``) and the level
    that its ``draw()`` is told; for a class with runtime parameters also ``par``, the float32 device row of the P
    parameters of the episode (or the env) that is drawn, which ``draw()`` sees as ``OsaDrawAt::par``."""
    cls: type
    level: int
    par: torch.Tensor | None = None


def row_floats(env_kind) -> int:
    """Leading floats of a state row that the kernel reads: SynthReach 6, the Goal families up to the last vase, the
    Circle families p and u; a custom class its TRACE."""
    if isinstance(env_kind, CustomScene):
        return env_kind.cls.trace_state_floats
    return 6 if env_kind == 1 else (4 if (env_kind // 16) % 2 == 0 else 52)


def camera_index(camera_name: str) -> int:
    if camera_name not in CAMERAS:
        raise ValueError(f'camera_name={camera_name!r}: one of {sorted(CAMERAS)}')
    return CAMERAS[camera_name]


def rasterise(env_kind: int | CustomScene, rows: torch.Tensor, offset: int, stride: int, first: int, count: int,
              trail: int, hit: torch.Tensor | None, camera: int, width: int, height: int, supersample: int,
              out: torch.Tensor | None = None) -> torch.Tensor:  # pylint: disable=too-many-locals
    """Frames first .. first + count - 1 of the episode whose record f has its state row at element
    ``offset + f * stride`` of the float32 device tensor ``rows``; ``hit``: uint8[>= first + count] on the device or
    None.  Returns (a view of ``out`` as) uint8 [count, height, width, 3] on the device."""
    lib = _lib.load(require_gpu=True)
    extra: tuple = ()
    if isinstance(env_kind, CustomScene):
        if not env_kind.cls.draws:
            raise ValueError(f'{env_kind.cls.struct} has no draw(): nothing to rasterise')
        entry, what = env_kind.cls.library().osa_custom_render_episode, env_kind.level
        if env_kind.cls.param_names:
            par = env_kind.par
            if par is None:
                raise ValueError(f'{env_kind.cls.struct} has runtime parameters: name the row to draw with '
                                 '(CustomScene.par)')
            assert par.dtype == torch.float32 and par.is_cuda and par.is_contiguous() \
                and par.numel() >= len(env_kind.cls.param_names)
            entry, extra = env_kind.cls.library().osa_custom_render_episode_params, (par.data_ptr(),)
    else:
        entry, what = lib.osa_render_episode, env_kind
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.is_cuda
    assert first >= 0 and count >= 1 and offset >= 0 and stride >= 0
    assert offset + (first + count - 1) * stride + row_floats(env_kind) <= rows.numel()
    assert hit is None or (hit.dtype == torch.uint8 and hit.is_contiguous() and hit.numel() >= first + count)
    n = count * height * width * 3
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=rows.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= n
    _lib.check(entry(int(what), rows.data_ptr() + 4 * offset, int(stride), int(first), int(count), int(trail),
                     _lib.ptr(hit), int(camera), int(width), int(height), int(supersample), out.data_ptr(), *extra,
                     _lib.stream_ptr()), entry.__name__)
    return out.reshape(-1)[:n].view(count, height, width, 3)


def stream_frames(env_kind: int | CustomScene, rows: torch.Tensor, offset: int, stride: int, frames: int,
                  trail: int, hit: torch.Tensor | None, camera: int, width: int, height: int, supersample: int,
                  frame_skip: int = 1, clock: dict | None = None):
    """Generator over numpy chunks [n, height, width, 3] of frames 0, frame_skip, 2 frame_skip, ... < ``frames``.
    ``clock`` (optional) accumulates the seconds spent in 'raster' (launch to completion) and 'copy' (device to pinned
    host)."""
    per = height * width * 3
    chunk = max(1, min(frames, CHUNK_BYTES // per))
    dev = torch.empty(chunk * per, dtype=torch.uint8, device=rows.device)
    host = torch.empty(chunk * per, dtype=torch.uint8, pin_memory=True)
    for first in range(0, frames, chunk):
        count = min(chunk, frames - first)
        t0 = time.perf_counter()
        rasterise(env_kind, rows, offset, stride, first, count, trail, hit, camera, width, height, supersample, dev)
        if clock is not None:
            torch.cuda.synchronize(rows.device)
        t1 = time.perf_counter()
        host[:count * per].copy_(dev[:count * per], non_blocking=True)
        torch.cuda.synchronize(rows.device)
        t2 = time.perf_counter()
        if clock is not None:
            clock['raster'] = clock.get('raster', 0.0) + (t1 - t0)
            clock['copy'] = clock.get('copy', 0.0) + (t2 - t1)
        keep = (-first) % frame_skip
        yield host[:count * per].view(count, height, width, 3).numpy()[keep::frame_skip]


__all__ = ['CAMERAS', 'CustomScene', 'camera_index', 'rasterise', 'stream_frames']
