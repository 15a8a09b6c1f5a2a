// SynthNavCircle{0,1,2}-v0's description with a draw() that states the circle picture (include/omnisafe_amd.h,
// osa_render_episode) through the generic scene rasteriser: the bytes must be those of the built-in kernel.
// Row: [0:2] p  [2:4] the heading u.  The cost region is painted as the arena in the cost colour with the free strip
// (level 1: |x| <= 0.75) or square (level 2: both axes) over it in the floor colour.
#pragma once
struct CircleDrawn : OsaPointCircle {
  static constexpr float DRAW_VIEW = 2.25f;
  static __device__ __forceinline__ void position(const float* rec, float& x, float& y) {
    x = rec[0];
    y = rec[1];
  }
  static __device__ __forceinline__ void draw(const float* rec, const OsaDrawAt& at, OsaScene& scene) {
    const float px = rec[0], py = rec[1];
    if (at.level == 0) {
      scene.box(-2.f, -2.f, 2.f, 2.f, OSA_COLOUR_FLOOR);
    } else {
      const float free_y = at.level == 2 ? 0.75f : 2.f;
      scene.box(-2.f, -2.f, 2.f, 2.f, OSA_COLOUR_COST);
      scene.box(-0.75f, -free_y, 0.75f, free_y, OSA_COLOUR_FLOOR);
    }
    scene.ring(0.f, 0.f, 0.9604f, 1.0404f, OSA_COLOUR_RING);
    scene.trail(0.0004f, OSA_COLOUR_TRAIL);
    scene.disc(px, py, 0.01f, at.hit ? OSA_COLOUR_HIT : OSA_COLOUR_POINT);
    scene.segment(px, py, px + 0.2f * rec[2], py + 0.2f * rec[3], 0.0009f, OSA_COLOUR_HEADING);
  }
};
