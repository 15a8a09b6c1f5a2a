// What the two rasterisers share: the palette and the two point-in-shape tests of the picture that
// include/omnisafe_amd.h (osa_render_episode) specifies.  render_kernels.hip draws the built-in families from a table
// of columns; scene_render.h draws whatever a description's draw() stages (include/omnisafe_amd_env.h).
// float32 + - * / and comparisons only, no fused multiply-adds: tests/render_twin.py reproduces every byte.
#pragma once
#include "osa_common.h"

// the palette, 0xRRGGBB (the table of include/omnisafe_amd.h and tests/render_twin.py), stated once:
// OSA_PAL_<NAME> is the index into OSA_RENDER_PALETTE, OSA_COLOUR_<NAME> the colour itself (what a draw() passes)
#define OSA_PALETTE(X)                                                                                       \
  X(OUTSIDE, 0x282C34) X(FLOOR, 0xECECE4) X(COST, 0xF4CCC4) X(RING, 0x60A060) X(HAZARD, 0x5A64DC)            \
  X(GOAL, 0x46BE5A) X(VASE, 0x50C8D2) X(TRAIL, 0xFAA028) X(POINT, 0xC82828) X(CAR, 0x8232AA) X(HIT, 0xFF00C8) \
  X(HEADING, 0x141414)
enum {
#define OSA_PAL_INDEX(NAME, RGB) OSA_PAL_##NAME,
  OSA_PALETTE(OSA_PAL_INDEX)
#undef OSA_PAL_INDEX
  OSA_PAL_COUNT
};
enum : unsigned {
#define OSA_PAL_COLOUR(NAME, RGB) OSA_COLOUR_##NAME = RGB,
  OSA_PALETTE(OSA_PAL_COLOUR)
#undef OSA_PAL_COLOUR
};
static __device__ const unsigned OSA_RENDER_PALETTE[OSA_PAL_COUNT] = {
#define OSA_PAL_ENTRY(NAME, RGB) RGB,
    OSA_PALETTE(OSA_PAL_ENTRY)
#undef OSA_PAL_ENTRY
};

#define OSA_RENDER_THREADS 256
#define OSA_RENDER_CHUNK 256  // trail segments staged per round (5 KB of LDS)

// The argument checks of osa_render_episode, stated once for both rasterisers: OSA_EINVAL before any launch.
static inline int osa_render_check(const float* state, const uint8_t* rgb, int first, int count, int trail, int camera,
                                   int width, int height, int supersample) {
  OSA_REQUIRE(state && rgb && (reinterpret_cast<uintptr_t>(rgb) & 3) == 0);
  OSA_REQUIRE(count >= 1 && first >= 0 && trail >= 0 && first <= 2147483647 - count);
  OSA_REQUIRE(width >= 4 && width <= 4096 && width % 4 == 0 && height >= 1 && height <= 4096);
  OSA_REQUIRE(supersample >= 1 && supersample <= 4 && (camera == 0 || camera == 1));
  return OSA_OK;
}

#pragma clang fp contract(off)
__device__ __forceinline__ bool osa_render_disc(float x, float y, float ox, float oy, float r2) {
  const float dx = x - ox, dy = y - oy;
  return dx * dx + dy * dy <= r2;
}

// The segment from (ax, ay) with extent (ex, ey) and squared length L2, at half-width sqrt(hw2).
__device__ __forceinline__ bool osa_render_segment(float x, float y, float ax, float ay, float ex, float ey, float L2,
                                                   float hw2) {
  const float wx = x - ax, wy = y - ay;
  float t = 0.f;
  if (L2 != 0.f) {
    t = (wx * ex + wy * ey) / L2;
    t = t < 0.f ? 0.f : t;
    t = t > 1.f ? 1.f : t;
  }
  const float dx = wx - t * ex, dy = wy - t * ey;
  return dx * dx + dy * dy <= hw2;
}
#pragma clang fp contract(fast)
