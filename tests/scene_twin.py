"""numpy float32 twin of the generic scene rasteriser (osa_custom_render_episode, csrc/scene_render.h): the picture
arithmetic of render_twin.py -- its rounding helpers, its sub-sample grid, its integer mean -- over a scene that a
Python ``draw(rec, level, hit) -> [primitives]`` states, as a description's draw() does on the device
(include/omnisafe_amd_env.h).  A primitive is a tuple, a colour an int 0xRRGGBB:

    ('disc', ox, oy, r2, colour)        ('ring', ox, oy, lo2, hi2, colour)      ('box', x0, y0, x1, y1, colour)
    ('segment', ax, ay, bx, by, hw2, colour)                                    ('trail', hw2, colour)

    render(draw, position, view, states[F, >= TRACE], first, count, trail, hit, camera, W, H, S, level=0, track=1.0)
        -> uint8[count, H, W, 3]

Below the twin: the draw() of the example headers tests/custom_envs/{reach,circle,ledge}_drawn.h and scene_caps.h,
restated.
"""
import numpy as np

import render_twin as R
from render_twin import F, add, mul, sub

DRAW_MAX = 64  # OSA_DRAW_MAX
COLOUR = {name: int(r) << 16 | int(g) << 8 | int(b) for name, (r, g, b) in zip(
    ('OUTSIDE', 'FLOOR', 'COST', 'RING', 'HAZARD', 'GOAL', 'VASE', 'TRAIL', 'POINT', 'CAR', 'HIT', 'HEADING'),
    R.PALETTE)}


def staged(prims):
    """The primitives that the scene keeps: a second trail is ignored, everything past DRAW_MAX is dropped."""
    kept, trail = [], False
    for prim in prims:
        if prim[0] == 'trail' and trail:
            continue
        if len(kept) >= DRAW_MAX:
            continue
        trail |= prim[0] == 'trail'
        kept.append(prim)
    return kept


def frame(draw, position, view, track, level, states, f, trail, was_hit, camera, W, H, S):
    rec = np.asarray(states[f], F)
    px, py = (F(v) for v in position(rec))
    cx, cy = (px, py) if camera else (F(0), F(0))
    half = F(track) if camera else F(view)
    h = (half / F(min(W, H) * S)).astype(F)
    u = (2 * np.arange(W * S) + 1 - W * S).astype(F)
    v = (H * S - 2 * np.arange(H * S) - 1).astype(F)
    x = np.broadcast_to(add(cx, mul(u, h))[None, :], (H * S, W * S))
    y = np.broadcast_to(add(cy, mul(v, h))[:, None], (H * S, W * S))
    c = np.full((H * S, W * S), COLOUR['OUTSIDE'], np.int64)
    for prim in staged(draw(rec, level, bool(was_hit))):
        kind, colour = prim[0], int(prim[-1])
        g = [F(t) for t in prim[1:-1]]
        if kind == 'disc':
            c[R.disc(x, y, g[0], g[1], g[2])] = colour
        elif kind == 'ring':
            dx, dy = sub(x, g[0]), sub(y, g[1])
            q2 = add(mul(dx, dx), mul(dy, dy))
            c[(g[2] <= q2) & (q2 <= g[3])] = colour
        elif kind == 'box':
            c[(g[0] <= x) & (x <= g[2]) & (g[1] <= y) & (y <= g[3])] = colour
        elif kind == 'segment':
            c[R.segment(x, y, g[0], g[1], sub(g[2], g[0]), sub(g[3], g[1]), g[4])] = colour
        elif kind == 'trail':
            on = np.zeros(c.shape, bool)
            for k in range(max(0, f - trail), f):
                (ax, ay), (bx, by) = position(np.asarray(states[k], F)), position(np.asarray(states[k + 1], F))
                on |= R.segment(x, y, F(ax), F(ay), sub(bx, ax), sub(by, ay), g[0])
            c[on] = colour
        else:
            raise ValueError(f'no primitive {kind!r}')
    rgb = np.stack([c >> 16, (c >> 8) & 255, c & 255], -1).astype(np.int32)
    rgb = rgb.reshape(H, S, W, S, 3).sum(axis=(1, 3))
    return ((rgb + S * S // 2) // (S * S)).astype(np.uint8)


def render(draw, position, view, states, first, count, trail, hit, camera, W, H, S, level=0, track=1.0):
    states = np.asarray(states, F)
    out = np.empty((count, H, W, 3), np.uint8)
    for n in range(count):
        f = first + n
        out[n] = frame(draw, position, view, track, level, states, f, trail, hit is not None and hit[f] != 0, camera,
                       W, H, S)
    return out


# ------------------------------------------------------------------ the example headers' draw(), restated
def position(rec):
    return rec[0], rec[1]


def reach_draw(rec, level, hit):
    C = COLOUR
    return [('box', -1.5, -1.5, 1.5, 1.5, C['FLOOR']), ('disc', rec[4], rec[5], 0.09, C['HAZARD']),
            ('disc', rec[2], rec[3], 0.0225, C['GOAL']), ('trail', 0.0004, C['TRAIL']),
            ('disc', rec[0], rec[1], 0.0025, C['HIT'] if hit else C['POINT'])]


def circle_draw(rec, level, hit):
    C = COLOUR
    px, py = rec[0], rec[1]
    if level == 0:
        ground = [('box', -2, -2, 2, 2, C['FLOOR'])]
    else:
        free_y = 0.75 if level == 2 else 2
        ground = [('box', -2, -2, 2, 2, C['COST']), ('box', -0.75, -free_y, 0.75, free_y, C['FLOOR'])]
    tip = add(px, mul(F(0.2), rec[2])), add(py, mul(F(0.2), rec[3]))
    return ground + [('ring', 0, 0, 0.9604, 1.0404, C['RING']), ('trail', 0.0004, C['TRAIL']),
                     ('disc', px, py, 0.01, C['HIT'] if hit else C['POINT']),
                     ('segment', px, py, tip[0], tip[1], 0.0009, C['HEADING'])]


LEDGE_VIEW, LEDGE_TRACK = 3.5, 1.5


def ledge_draw(rec, level, hit):
    C = COLOUR
    px, py = rec[0], rec[1]
    prims = [('box', -0.5, -1, 3, 1, C['FLOOR'])]
    if level >= 1:
        prims += [('box', -0.5, 0.5, 3, 1, C['COST']), ('box', -0.5, -1, 3, -0.5, C['COST'])]
    tip = add(px, mul(F(4), rec[2])), add(py, mul(F(4), rec[3]))
    return prims + [('box', 3, -1, 3.4, 1, C['GOAL']), ('segment', -0.5, 0, 3, 0, 0.01, 0x9098A0),
                    ('trail', 0.0009, C['TRAIL']), ('ring', px, py, 0.04, 0.0625, C['HIT'] if hit else 0x3070C0),
                    ('disc', px, py, 0.01, C['POINT']), ('segment', px, py, tip[0], tip[1], 0.0004, C['HEADING'])]


def caps_draw(n):
    """scene_caps.h: n cells of the 8 x 8 grid, then (DrawOver) three primitives that would cover everything."""
    def draw(rec, level, hit):
        prims = []
        for k in range(min(n, DRAW_MAX)):
            x0, y0 = add(F(-2), mul(F(0.5), F(k % 8))), add(F(-2), mul(F(0.5), F(k // 8)))
            prims.append(('box', add(x0, F(0.0625)), add(y0, F(0.0625)), add(x0, F(0.4375)), add(y0, F(0.4375)),
                          0x010203 * (k + 1)))
        if n > DRAW_MAX:
            prims += [('box', -3, -3, 3, 3, COLOUR['HIT']), ('trail', 9, COLOUR['TRAIL']),
                      ('disc', 0, 0, 9, COLOUR['CAR'])]
        return prims
    return draw
