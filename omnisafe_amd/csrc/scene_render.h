// The generic scene rasteriser: osa_render_episode's picture arithmetic (include/omnisafe_amd.h) over a scene that a
// description's draw() states (include/omnisafe_amd_env.h), as render_kernels.hip does it over a table of columns for
// the built-in families.  Instantiated per description by csrc/custom/custom_env.hip.
//
// Mapping (render_kernels.hip's): a workgroup of 256 lanes draws 1024 consecutive row-major pixels of ONE frame, lane l
// the 4 horizontally adjacent pixels 4 l .. 4 l + 3, one 12-byte store per lane.  Workgroups share nothing and write
// disjoint bytes: no atomics, no flags.
// Staging: the frame's record goes to LDS, and with it the episode's parameter row (a description with PARAMS); ONE lane runs E::draw on it, which appends primitives to the OsaScene in LDS
// (kind, colour, geometry; a segment's extent and squared length computed there, once); barrier; where the scene has a
// trail, its segments are staged in chunks of OSA_RENDER_CHUNK and collected into a per-lane bit mask; then every lane
// walks the primitive list once, testing its 4 S^2 sub-samples against each primitive.  At every step of the walk all
// lanes read the same LDS addresses (broadcast reads: no bank conflicts whatever the layout) and the kind is made
// wave-uniform (readfirstlane), so the dispatch is a scalar branch and no lane diverges on the scene.
#pragma once
#include <type_traits>
#include <utility>

#include "env_params.h"
#include "render_common.h"

#define OSA_DRAW_MAX 64  // primitives of a scene; 2 KB of LDS.  The widest built-in picture (Goal2) has 25.

struct OsaDrawAt {
  int level;  // the level the caller named
  int hit;    // the caller's hit[f] != 0 (the evaluator: the step into this record cost something)
  int frame;  // f, the index of the record
  const float* par;  // the P parameters of the episode the record is of; nullptr for a description without PARAMS
};

enum { OSA_PRIM_DISC, OSA_PRIM_RING, OSA_PRIM_BOX, OSA_PRIM_SEGMENT, OSA_PRIM_TRAIL };

#pragma clang fp contract(off)
// What draw() paints on: primitives in painter's order.  Lives in LDS; the members are the kernel's, a description
// calls the five functions only.
struct OsaScene {
  int count;     // primitives staged, <= OSA_DRAW_MAX
  int trail_at;  // index of the trail primitive; -1: none
  int kind[OSA_DRAW_MAX];
  unsigned colour[OSA_DRAW_MAX];
  alignas(16) float geo[OSA_DRAW_MAX][4];  // disc: ox oy r2 | ring: ox oy lo2 hi2 | box: x0 y0 x1 y1 | segment: ax ay ex ey
  alignas(8) float ext[OSA_DRAW_MAX][2];   // segment: L2 hw2 | trail: hw2

  __device__ __forceinline__ void clear() {
    count = 0;
    trail_at = -1;
  }
  // (a primitive past the cap is dropped)
  __device__ __forceinline__ int stage(int k, unsigned c, float g0, float g1, float g2, float g3, float e0, float e1) {
    const int at = count;
    if (at >= OSA_DRAW_MAX) return -1;
    kind[at] = k;
    colour[at] = c;
    geo[at][0] = g0; geo[at][1] = g1; geo[at][2] = g2; geo[at][3] = g3;
    ext[at][0] = e0; ext[at][1] = e1;
    count = at + 1;
    return at;
  }
  __device__ __forceinline__ void disc(float ox, float oy, float r2, unsigned c) {
    stage(OSA_PRIM_DISC, c, ox, oy, r2, 0.f, 0.f, 0.f);
  }
  __device__ __forceinline__ void ring(float ox, float oy, float lo2, float hi2, unsigned c) {
    stage(OSA_PRIM_RING, c, ox, oy, lo2, hi2, 0.f, 0.f);
  }
  __device__ __forceinline__ void box(float x0, float y0, float x1, float y1, unsigned c) {
    stage(OSA_PRIM_BOX, c, x0, y0, x1, y1, 0.f, 0.f);
  }
  __device__ __forceinline__ void segment(float ax, float ay, float bx, float by, float hw2, unsigned c) {
    const float ex = bx - ax, ey = by - ay;
    stage(OSA_PRIM_SEGMENT, c, ax, ay, ex, ey, ex * ex + ey * ey, hw2);
  }
  // (at most once: a second call is ignored, and so is one past the cap)
  __device__ __forceinline__ void trail(float hw2, unsigned c) {
    if (trail_at < 0) trail_at = stage(OSA_PRIM_TRAIL, c, 0.f, 0.f, 0.f, 0.f, hw2, 0.f);
  }
};
#pragma clang fp contract(fast)

// Whether a description draws: draw() callable as stated.  (What else a drawing description needs -- position(),
// DRAW_VIEW, TRACE >= 1 -- is custom_env.hip's to demand, with a message each.)
template <class E, class = void>
struct OsaHasDraw : std::false_type {};
template <class E>
struct OsaHasDraw<E, std::void_t<decltype(E::draw((const float*)nullptr, std::declval<const OsaDrawAt&>(),
                                                  std::declval<OsaScene&>()))>> : std::true_type {};
template <class E, class = void>
struct OsaHasPosition : std::false_type {};
template <class E>
struct OsaHasPosition<E, std::void_t<decltype(E::position((const float*)nullptr, std::declval<float&>(),
                                                          std::declval<float&>()))>> : std::true_type {};
template <class E, class = void>
struct OsaHasDrawView : std::false_type {};
template <class E>
struct OsaHasDrawView<E, std::void_t<decltype(E::DRAW_VIEW)>> : std::true_type {};
template <class E, class = void>
struct OsaDrawTrack {
  static constexpr float value = 1.f;
};
template <class E>
struct OsaDrawTrack<E, std::void_t<decltype(E::DRAW_TRACK)>> {
  static constexpr float value = E::DRAW_TRACK;
};

struct OsaSceneArgs {
  const float* state;
  long stride;
  int first, count, trail;
  const uint8_t* hit;
  int camera, width, height;
  uint8_t* rgb;
  int level;
  int quads;  // width * height / 4
  int blocks_per_frame;
  const float* par;  // the episode's parameter row (a description with PARAMS: P floats), else nullptr
};

#pragma clang fp contract(off)
__device__ __forceinline__ bool osa_scene_ring(float x, float y, float ox, float oy, float lo2, float hi2) {
  const float dx = x - ox, dy = y - oy;
  const float q2 = dx * dx + dy * dy;
  return lo2 <= q2 && q2 <= hi2;
}

template <class E, int S>
__global__ __launch_bounds__(OSA_RENDER_THREADS) void osa_scene_render_kernel(OsaSceneArgs a) {
  __shared__ float rec_s[E::TRACE];
  __shared__ OsaScene scene;
  __shared__ float4 seg[OSA_RENDER_CHUNK];  // ax, ay, ex, ey
  __shared__ float seg_l2[OSA_RENDER_CHUNK];
  const int local = blockIdx.x / a.blocks_per_frame;  // frame of this workgroup, uniform
  const int f = a.first + local;
  const int quad = (blockIdx.x - local * a.blocks_per_frame) * OSA_RENDER_THREADS + threadIdx.x;
  const bool active = quad < a.quads;
  const float* __restrict__ rec = a.state + (long)f * a.stride;
  for (int c = threadIdx.x; c < E::TRACE; c += OSA_RENDER_THREADS) rec_s[c] = rec[c];  // (TRACE reaches 256)
  constexpr int P = OsaEnvParams<E>::value;
  __shared__ float par_s[P > 0 ? P : 1];
  if constexpr (P > 0) {
    if ((int)threadIdx.x < P) par_s[threadIdx.x] = a.par[threadIdx.x];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    scene.clear();
    const OsaDrawAt at = {a.level, a.hit != nullptr && a.hit[f] != 0 ? 1 : 0, f, P > 0 ? par_s : nullptr};
    E::draw(rec_s, at, scene);
  }
  __syncthreads();

  const int wq = a.width >> 2;
  const int i = quad / wq, j0 = (quad - i * wq) * 4;
  float px, py;
  E::position(rec_s, px, py);
  const float cx = a.camera ? px : 0.f, cy = a.camera ? py : 0.f;
  const int m = a.width < a.height ? a.width : a.height;
  const float half = a.camera ? OsaDrawTrack<E>::value : (float)E::DRAW_VIEW;
  const float h = half / (float)(m * S);
  const int us = a.width * S, vs = a.height * S;
  float xs[4 * S], ys[S];  // sub-sample (sa, sb) of pixel j0 + p is (xs[p * S + sb], ys[sa])
#pragma unroll
  for (int q = 0; q < 4 * S; ++q) xs[q] = cx + (float)(2 * (j0 * S + q) + 1 - us) * h;
#pragma unroll
  for (int sa = 0; sa < S; ++sa) ys[sa] = cy + (float)(vs - 2 * (i * S + sa) - 1) * h;

  // the trail first, where the scene has one: bit (p * S + sa) * S + sb of `on_trail` says that sub-sample (sa, sb) of
  // pixel j0 + p lies on the path through position() of records max(0, f - trail) .. f
  unsigned long long on_trail = 0;
  const int trail_at = __builtin_amdgcn_readfirstlane(scene.trail_at);
  if (trail_at >= 0) {
    const float hw2 = scene.ext[trail_at][0];
    const int lo = f - a.trail > 0 ? f - a.trail : 0;
    for (int base = lo; base < f; base += OSA_RENDER_CHUNK) {
      const int n = f - base < OSA_RENDER_CHUNK ? f - base : OSA_RENDER_CHUNK;
      __syncthreads();  // the previous chunk has been read
      if ((int)threadIdx.x < n) {
        const float* __restrict__ s0 = a.state + (long)(base + threadIdx.x) * a.stride;
        float ax, ay, bx, by;
        E::position(s0, ax, ay);
        E::position(s0 + a.stride, bx, by);
        const float ex = bx - ax, ey = by - ay;
        seg[threadIdx.x] = make_float4(ax, ay, ex, ey);
        seg_l2[threadIdx.x] = ex * ex + ey * ey;
      }
      __syncthreads();
      if (active) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int sa = 0; sa < S; ++sa)
#pragma unroll
            for (int sb = 0; sb < S; ++sb) {
              const int bit = (p * S + sa) * S + sb;
              bool on = (on_trail >> bit) & 1;
              for (int s = 0; s < n && !on; ++s) {
                const float4 g = seg[s];
                on = osa_render_segment(xs[p * S + sb], ys[sa], g.x, g.y, g.z, g.w, seg_l2[s], hw2);
              }
              on_trail |= (unsigned long long)on << bit;
            }
      }
    }
  }
  if (!active) return;

  // the walk: one primitive at a time over all sub-samples of the quad; a later primitive wins
  unsigned c[4 * S * S];
#pragma unroll
  for (int q = 0; q < 4 * S * S; ++q) c[q] = OSA_COLOUR_OUTSIDE;
  const int count = __builtin_amdgcn_readfirstlane(scene.count);
  for (int k = 0; k < count; ++k) {
    const int kind = __builtin_amdgcn_readfirstlane(scene.kind[k]);
    const unsigned col = (unsigned)__builtin_amdgcn_readfirstlane((int)scene.colour[k]);
    const float g0 = scene.geo[k][0], g1 = scene.geo[k][1], g2 = scene.geo[k][2], g3 = scene.geo[k][3];
    const float e0 = scene.ext[k][0], e1 = scene.ext[k][1];
#define OSA_SCENE_EACH(TEST)                                      \
  _Pragma("unroll") for (int p = 0; p < 4; ++p)                   \
  _Pragma("unroll") for (int sa = 0; sa < S; ++sa)                \
  _Pragma("unroll") for (int sb = 0; sb < S; ++sb) {              \
    const float x = xs[p * S + sb], y = ys[sa];                   \
    (void)x; (void)y;                                             \
    const int bit = (p * S + sa) * S + sb;                        \
    if (TEST) c[bit] = col;                                       \
  }
    switch (kind) {
      case OSA_PRIM_DISC:
        OSA_SCENE_EACH(osa_render_disc(x, y, g0, g1, g2))
        break;
      case OSA_PRIM_RING:
        OSA_SCENE_EACH(osa_scene_ring(x, y, g0, g1, g2, g3))
        break;
      case OSA_PRIM_BOX:
        OSA_SCENE_EACH(g0 <= x && x <= g2 && g1 <= y && y <= g3)
        break;
      case OSA_PRIM_SEGMENT:
        OSA_SCENE_EACH(osa_render_segment(x, y, g0, g1, g2, g3, e0, e1))
        break;
      default:  // OSA_PRIM_TRAIL
        OSA_SCENE_EACH((on_trail >> bit) & 1)
        break;
    }
#undef OSA_SCENE_EACH
  }

  unsigned out[3] = {0, 0, 0};  // the 12 bytes of the quad
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int sum_r = 0, sum_g = 0, sum_b = 0;
#pragma unroll
    for (int q = 0; q < S * S; ++q) {
      const unsigned col = c[p * S * S + q];
      sum_r += (int)(col >> 16);
      sum_g += (int)((col >> 8) & 255u);
      sum_b += (int)(col & 255u);
    }
    const unsigned ch[3] = {(unsigned)((sum_r + S * S / 2) / (S * S)), (unsigned)((sum_g + S * S / 2) / (S * S)),
                            (unsigned)((sum_b + S * S / 2) / (S * S))};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int byte = 3 * p + k;
      out[byte >> 2] |= ch[k] << (8 * (byte & 3));
    }
  }
  struct alignas(4) Quad { unsigned d[3]; };
  Quad* __restrict__ dst = reinterpret_cast<Quad*>(a.rgb + ((size_t)local * a.quads + quad) * 12);
  *dst = Quad{{out[0], out[1], out[2]}};
}
#pragma clang fp contract(fast)

// osa_custom_render_episode behind its level check: osa_render_episode's argument checks, then one launch.  par: the
// episode's parameter row for a description with PARAMS (the caller has checked it), else nullptr.
template <class E>
static int osa_scene_render_launch(int level, const float* state, long stride, int first, int count, int trail,
                                   const uint8_t* hit, int camera, int width, int height, int supersample,
                                   uint8_t* rgb, const float* par, void* stream) {
  OsaSceneArgs a = {state, stride, first, count, trail, hit, camera, width, height, rgb, level, width * height / 4, 0,
                    par};
  a.blocks_per_frame = (a.quads + OSA_RENDER_THREADS - 1) / OSA_RENDER_THREADS;
  if ((long)count * a.blocks_per_frame > 2147483647L) return OSA_EUNSUPPORTED;  // render in chunks of frames
  const dim3 grid((unsigned)((long)count * a.blocks_per_frame)), block(OSA_RENDER_THREADS);
  switch (supersample) {
    case 1: hipLaunchKernelGGL((osa_scene_render_kernel<E, 1>), grid, block, 0, osa_stream(stream), a); break;
    case 2: hipLaunchKernelGGL((osa_scene_render_kernel<E, 2>), grid, block, 0, osa_stream(stream), a); break;
    case 3: hipLaunchKernelGGL((osa_scene_render_kernel<E, 3>), grid, block, 0, osa_stream(stream), a); break;
    default: hipLaunchKernelGGL((osa_scene_render_kernel<E, 4>), grid, block, 0, osa_stream(stream), a); break;
  }
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}
