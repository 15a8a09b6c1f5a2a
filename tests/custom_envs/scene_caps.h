// Test-only descriptions for the size of a scene (OSA_DRAW_MAX = 64): SynthReach-v0's env with a draw() that appends
// nothing, exactly OSA_DRAW_MAX primitives, and three more than that.  Primitive k < 64 is the box of cell (k % 8,
// k / 8) of an 8 x 8 grid over [-2, 2]^2 in the colour 0x010203 * (k + 1); the three past the cap would cover
// everything.  tests/test_custom_render_gpu.py restates them in Python.
#pragma once
struct SceneCapsBase : OsaReachEnv {
  static constexpr float DRAW_VIEW = 2.f;
  static __device__ __forceinline__ void position(const float* rec, float& x, float& y) {
    x = rec[0];
    y = rec[1];
  }
  static __device__ __forceinline__ void cells(OsaScene& scene, int n) {
    for (int k = 0; k < n; ++k) {
      const float x0 = -2.f + 0.5f * (float)(k % 8), y0 = -2.f + 0.5f * (float)(k / 8);
      scene.box(x0 + 0.0625f, y0 + 0.0625f, x0 + 0.4375f, y0 + 0.4375f, 0x010203u * (unsigned)(k + 1));
    }
  }
};
struct DrawNothing : SceneCapsBase {
  static __device__ __forceinline__ void draw(const float*, const OsaDrawAt&, OsaScene&) {}
};
struct DrawFull : SceneCapsBase {
  static __device__ __forceinline__ void draw(const float*, const OsaDrawAt&, OsaScene& scene) {
    cells(scene, OSA_DRAW_MAX);
  }
};
struct DrawOver : SceneCapsBase {
  static __device__ __forceinline__ void draw(const float*, const OsaDrawAt&, OsaScene& scene) {
    cells(scene, OSA_DRAW_MAX);
    scene.box(-3.f, -3.f, 3.f, 3.f, OSA_COLOUR_HIT);
    scene.trail(9.f, OSA_COLOUR_TRAIL);
    scene.disc(0.f, 0.f, 9.f, OSA_COLOUR_CAR);
  }
};
