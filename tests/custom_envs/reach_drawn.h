// SynthReach-v0's description with a draw() that states SynthReach's picture (include/omnisafe_amd.h,
// osa_render_episode) through the generic scene rasteriser: the bytes must be those of the built-in kernel.
// Row: [0:2] p  [2:4] goal  [4:6] hazard.
#pragma once
struct ReachDrawn : OsaReachEnv {
  static constexpr float DRAW_VIEW = 1.75f;
  static __device__ __forceinline__ void position(const float* rec, float& x, float& y) {
    x = rec[0];
    y = rec[1];
  }
  static __device__ __forceinline__ void draw(const float* rec, const OsaDrawAt& at, OsaScene& scene) {
    scene.box(-1.5f, -1.5f, 1.5f, 1.5f, OSA_COLOUR_FLOOR);
    scene.disc(rec[4], rec[5], 0.09f, OSA_COLOUR_HAZARD);
    scene.disc(rec[2], rec[3], 0.0225f, OSA_COLOUR_GOAL);
    scene.trail(0.0004f, OSA_COLOUR_TRAIL);
    scene.disc(rec[0], rec[1], 0.0025f, at.hit ? OSA_COLOUR_HIT : OSA_COLOUR_POINT);
  }
};
