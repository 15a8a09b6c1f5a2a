// The Ledge (ledge.h) with a picture of its own, for the tests of the generic scene rasteriser: every primitive kind,
// the level and `hit`, a view and a tracking view that are not the built-in ones, and two colours outside the palette.
// Record (TRACE = 5): [0:2] p  [2:4] v  [4] steps.  tests/test_custom_render_gpu.py restates this draw() in Python.
#pragma once
#include "ledge.h"

struct LedgeDrawn : Ledge {
  static constexpr float DRAW_VIEW = 3.5f, DRAW_TRACK = 1.5f;
  static __device__ __forceinline__ void position(const float* rec, float& x, float& y) {
    x = rec[0];
    y = rec[1];
  }
  static __device__ __forceinline__ void draw(const float* rec, const OsaDrawAt& at, OsaScene& scene) {
    const float px = rec[0], py = rec[1];
    scene.box(-0.5f, -1.f, 3.f, 1.f, OSA_COLOUR_FLOOR);  // the ledge
    if (at.level >= 1) {                                 // where walking costs
      scene.box(-0.5f, 0.5f, 3.f, 1.f, OSA_COLOUR_COST);
      scene.box(-0.5f, -1.f, 3.f, -0.5f, OSA_COLOUR_COST);
    }
    scene.box(3.f, -1.f, 3.4f, 1.f, OSA_COLOUR_GOAL);  // arrived
    scene.segment(-0.5f, 0.f, 3.f, 0.f, 0.01f, 0x9098A0);  // the centre line
    scene.trail(0.0009f, OSA_COLOUR_TRAIL);
    scene.ring(px, py, 0.04f, 0.0625f, at.hit ? OSA_COLOUR_HIT : 0x3070C0);  // a halo around the walker
    scene.disc(px, py, 0.01f, OSA_COLOUR_POINT);
    scene.segment(px, py, px + 4.f * rec[2], py + 4.f * rec[3], 0.0004f, OSA_COLOUR_HEADING);  // its velocity
  }
};
