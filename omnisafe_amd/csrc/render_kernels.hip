// Rasterised replays of the geometric device envs (osa_render_episode): frames of a top-down picture of the state rows
// that osa_eval_episodes and the per-step evaluator trace.  The picture is a specification of this package, stated in
// include/omnisafe_amd.h (osa_render_episode) and restated in numpy by tests/render_twin.py; float32 + - * / and
// comparisons only, no fused multiply-adds, so the twin reproduces every byte.
//
// Mapping: a workgroup of 256 lanes draws 1024 consecutive pixels (row-major) of ONE frame, lane l the 4 horizontally
// adjacent pixels 4 l .. 4 l + 3 of that run (width % 4 == 0: a quad never crosses a row), and writes their 12 bytes
// with one dwordx3 store -- consecutive lanes write consecutive 12-byte pieces.  The frame index is uniform in the
// workgroup, which stages the frame's scene once in LDS: the state row of the frame's record and, in chunks of
// OSA_RENDER_CHUNK segments, the trail (start, extent and squared length of every segment, computed once by one lane
// each).  Workgroups share nothing and write disjoint bytes: no atomics, no flags, no order between workgroups.
#include "render_common.h"  // the palette, osa_render_disc, osa_render_segment, the argument checks

#define OSA_RENDER_ROW 64     // floats of the widest state row

struct OsaRenderArgs {
  const float* state;
  long stride;
  int first, count, trail;
  const uint8_t* hit;
  int camera, width, height;
  uint8_t* rgb;
  int row_floats;          // floats of the state row that the picture reads
  float arena, half;       // half-width of the arena and of the camera's view
  int circle, level;       // circle task (cost region and ring) and its level
  int goal_col;            // column of the goal in the row; -1: none
  int haz_col, hazards;    // first hazard column and the number of hazards
  int vase_col, vases;
  float haz_r2, goal_r2, robot_r2;
  int heading;             // the row has a heading u in columns 2, 3
  int robot_colour;
  int quads;               // width * height / 4
  int blocks_per_frame;
};

#pragma clang fp contract(off)
template <int S>
__global__ __launch_bounds__(OSA_RENDER_THREADS) void osa_render_kernel(OsaRenderArgs a) {
  __shared__ float row[OSA_RENDER_ROW];
  __shared__ float4 seg[OSA_RENDER_CHUNK];   // ax, ay, ex, ey
  __shared__ float seg_l2[OSA_RENDER_CHUNK];
  const int local = blockIdx.x / a.blocks_per_frame;  // frame of this workgroup, uniform
  const int f = a.first + local;
  const int quad = (blockIdx.x - local * a.blocks_per_frame) * OSA_RENDER_THREADS + threadIdx.x;
  const bool active = quad < a.quads;
  const float* __restrict__ rec = a.state + (long)f * a.stride;
  if ((int)threadIdx.x < a.row_floats) row[threadIdx.x] = rec[threadIdx.x];
  __syncthreads();
  const int wq = a.width >> 2;
  const int i = quad / wq, j0 = (quad - i * wq) * 4;
  const float px = row[0], py = row[1];
  const float cx = a.camera ? px : 0.f, cy = a.camera ? py : 0.f;
  const int m = a.width < a.height ? a.width : a.height;
  const float h = a.half / (float)(m * S);
  const int us = a.width * S, vs = a.height * S;

  // layer 7 first: bit (p * S + sa) * S + sb of `on_trail` says that sub-sample (sa, sb) of pixel j0 + p lies on the
  // trail through records max(0, f - trail) .. f
  unsigned long long on_trail = 0;
  const int lo = f - a.trail > 0 ? f - a.trail : 0;
  for (int base = lo; base < f; base += OSA_RENDER_CHUNK) {
    const int n = f - base < OSA_RENDER_CHUNK ? f - base : OSA_RENDER_CHUNK;
    __syncthreads();  // the previous chunk has been read
    if ((int)threadIdx.x < n) {
      const float* __restrict__ s0 = a.state + (long)(base + threadIdx.x) * a.stride;
      const float* __restrict__ s1 = s0 + a.stride;
      const float ax = s0[0], ay = s0[1];
      const float ex = s1[0] - ax, ey = s1[1] - ay;
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
            const float x = cx + (float)(2 * ((j0 + p) * S + sb) + 1 - us) * h;
            const float y = cy + (float)(vs - 2 * (i * S + sa) - 1) * h;
            bool on = (on_trail >> bit) & 1;
            for (int s = 0; s < n && !on; ++s) {
              const float4 g = seg[s];
              on = osa_render_segment(x, y, g.x, g.y, g.z, g.w, seg_l2[s], 0.0004f);
            }
            on_trail |= (unsigned long long)on << bit;
          }
    }
  }
  if (!active) return;

  const bool was_hit = a.hit != nullptr && a.hit[f] != 0;
  const int robot = was_hit ? OSA_PAL_HIT : a.robot_colour;
  float hex = 0.f, hey = 0.f, hl2 = 0.f;
  if (a.heading) {
    const float tx = px + 0.2f * row[2], ty = py + 0.2f * row[3];
    hex = tx - px;
    hey = ty - py;
    hl2 = hex * hex + hey * hey;
  }
  unsigned out[3] = {0, 0, 0};  // the 12 bytes of the quad
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int sum_r = 0, sum_g = 0, sum_b = 0;
#pragma unroll
    for (int sa = 0; sa < S; ++sa)
#pragma unroll
      for (int sb = 0; sb < S; ++sb) {
        const float x = cx + (float)(2 * ((j0 + p) * S + sb) + 1 - us) * h;
        const float y = cy + (float)(vs - 2 * (i * S + sa) - 1) * h;
        const float absx = x < 0.f ? -x : x, absy = y < 0.f ? -y : y;
        const bool inside = absx <= a.arena && absy <= a.arena;
        int c = inside ? OSA_PAL_FLOOR : OSA_PAL_OUTSIDE;
        if (a.circle) {
          if (inside && ((a.level >= 1 && absx > 0.75f) || (a.level == 2 && absy > 0.75f))) c = OSA_PAL_COST;
          const float q2 = x * x + y * y;
          if (q2 >= 0.9604f && q2 <= 1.0404f) c = OSA_PAL_RING;
        }
        for (int k = 0; k < a.hazards; ++k)
          if (osa_render_disc(x, y, row[a.haz_col + 2 * k], row[a.haz_col + 2 * k + 1], a.haz_r2)) c = OSA_PAL_HAZARD;
        if (a.goal_col >= 0 && osa_render_disc(x, y, row[a.goal_col], row[a.goal_col + 1], a.goal_r2))
          c = OSA_PAL_GOAL;
        for (int k = 0; k < a.vases; ++k)
          if (osa_render_disc(x, y, row[a.vase_col + 2 * k], row[a.vase_col + 2 * k + 1], 0.01f)) c = OSA_PAL_VASE;
        if ((on_trail >> ((p * S + sa) * S + sb)) & 1) c = OSA_PAL_TRAIL;
        if (osa_render_disc(x, y, px, py, a.robot_r2)) c = robot;
        if (a.heading && osa_render_segment(x, y, px, py, hex, hey, hl2, 0.0009f)) c = OSA_PAL_HEADING;
        const unsigned col = OSA_RENDER_PALETTE[c];
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

extern "C" {

int osa_render_episode(int env_kind, const float* state, long stride, int first, int count, int trail,
                       const uint8_t* hit, int camera, int width, int height, int supersample, uint8_t* rgb,
                       void* stream) {
  const int rc = osa_render_check(state, rgb, first, count, trail, camera, width, height, supersample);
  if (rc != OSA_OK) return rc;
  OsaRenderArgs a = {};
  const bool reach = env_kind == OSA_EVAL_ENV_REACH;
  const int families[4] = {OSA_EVAL_ENV_NAV0, OSA_EVAL_ENV_CIRCLE0, OSA_EVAL_ENV_CARGOAL0, OSA_EVAL_ENV_CARCIRCLE0};
  int family = -1;
  for (int k = 0; k < 4; ++k)
    if (env_kind >= families[k] && env_kind <= families[k] + 2) family = k;
  if (!reach && family < 0) return OSA_EUNSUPPORTED;
  a.level = reach ? 0 : env_kind - families[family];
  a.goal_col = -1;
  if (reach) {  // row: p, goal, hazard
    a.row_floats = 6; a.arena = 1.5f; a.half = 1.75f; a.goal_col = 2; a.goal_r2 = 0.0225f;
    a.haz_col = 4; a.hazards = 1; a.haz_r2 = 0.09f; a.robot_r2 = 0.0025f; a.robot_colour = OSA_PAL_POINT;
  } else {
    a.arena = 2.f; a.half = 2.25f; a.heading = 1; a.robot_r2 = 0.01f;
    a.robot_colour = (family & 2) ? OSA_PAL_CAR : OSA_PAL_POINT;
    a.circle = family & 1;
    a.row_floats = 4;
    if (!a.circle) {  // row: p u . . . . goal . . hazards from 12, vases from 32 (osa_nav_hazards / osa_nav_vases)
      a.row_floats = 52; a.goal_col = 8; a.goal_r2 = 0.09f; a.haz_col = 12; a.haz_r2 = 0.04f; a.vase_col = 32;
      a.hazards = a.level == 0 ? 0 : (a.level == 1 ? 8 : 10);
      a.vases = a.level == 0 ? 0 : (a.level == 1 ? 1 : 10);
    }
  }
  if (camera == 1) a.half = 1.f;
  a.state = state; a.stride = stride; a.first = first; a.count = count; a.trail = trail; a.hit = hit;
  a.camera = camera; a.width = width; a.height = height; a.rgb = rgb;
  a.quads = width * height / 4;
  a.blocks_per_frame = (a.quads + OSA_RENDER_THREADS - 1) / OSA_RENDER_THREADS;
  if ((long)count * a.blocks_per_frame > 2147483647L) return OSA_EUNSUPPORTED;  // render in chunks of frames
  const dim3 grid((unsigned)((long)count * a.blocks_per_frame));
  switch (supersample) {
    case 1: hipLaunchKernelGGL(osa_render_kernel<1>, grid, dim3(OSA_RENDER_THREADS), 0, osa_stream(stream), a); break;
    case 2: hipLaunchKernelGGL(osa_render_kernel<2>, grid, dim3(OSA_RENDER_THREADS), 0, osa_stream(stream), a); break;
    case 3: hipLaunchKernelGGL(osa_render_kernel<3>, grid, dim3(OSA_RENDER_THREADS), 0, osa_stream(stream), a); break;
    default: hipLaunchKernelGGL(osa_render_kernel<4>, grid, dim3(OSA_RENDER_THREADS), 0, osa_stream(stream), a); break;
  }
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

}  // extern "C"
