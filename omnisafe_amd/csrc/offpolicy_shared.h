// What the off-policy steps share (td3_kernels.hip: TD3 / DDPG, sac_kernels.hip: SAC): the gather of the minibatch rows
// from the replay ring, the data gradient of a critic down to its input rows, the fixed-order gradient norm with the L2
// term, Adam with the clip scale, the Polyak update and the statistics, and the step counter.  Moved here unchanged from
// td3_kernels.hip; both translation units include it and get their own instantiations.
#pragma once
#include <math.h>

#include "chain_layer.h"

namespace {

constexpr int T_NB = 32;  // workgroups (= partial sums) of a gradient-norm reduction

// ddpg.py:426: reward + gamma (1 - done) q
__device__ __forceinline__ float td3_y(float sig, float done, float gamma, float q) {
  return __fadd_rn(sig, __fmul_rn(__fmul_rn(gamma, 1.f - done), q));
}

int td3_ring_ok(const osa_td3_ring* r, int D, int A) {
  return r && r->obs && r->act && r->reward && r->cost && r->done && r->next_obs && r->pos && r->size >= 1 &&
         r->ld_obs >= D && r->ld_act >= A;
}

// ---- the layer route's gather ----------------------------------------------------------------------------------------
struct TGather {
  osa_td3_ring r;
  const long* idx;
  const long* step;
  int nslots, B, D, A, ldsa;
  float *xq, *xn0, *xn1, *rcd;
};
__global__ __launch_bounds__(256) void td3_gather_kernel(TGather g) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
  if (b >= g.B) return;
  long i = g.idx[(*g.step % g.nslots) * g.B + b];
  if (i < 0 || i >= g.r.size) i = 0;
  const float* o = g.r.obs + i * g.r.ld_obs;
  const float* a = g.r.act + i * g.r.ld_act;
  const float* nx = g.r.next_obs + i * g.r.ld_obs;
  for (int c = t; c < g.ldsa; c += 64) {
    g.xq[(long)b * g.ldsa + c] = c < g.D ? o[c] : (c < g.D + g.A ? a[c - g.D] : 0.f);
    const float v = c < g.D ? nx[c] : 0.f;
    g.xn0[(long)b * g.ldsa + c] = v;
    if (g.xn1) g.xn1[(long)b * g.ldsa + c] = v;
  }
  if (t == 0) {
    g.rcd[b] = g.r.reward[i];
    g.rcd[g.B + b] = g.r.cost[i];
    g.rcd[2 * g.B + b] = g.r.done[i];
  }
}

// the data gradient of a critic down to its input rows: dx[B][ldsa] = dL/d(obs || a)
int td3_critic_dx(const CNet& n, const float* params, const size_t* h, const size_t* z, size_t dx, int B, int ldsa,
                  float* ws, hipStream_t st) {
  int cur = 0;
  for (int l = n.L - 1; l >= 0; --l) {
    GArgs gd = {};
    gd.splits = 1;
    GProb q = crr_prob();  // dZ_{l-1}[rows][in] = (dZ_l[rows][out] . W_l[out][in]) * act'(H_{l-1})
    q.A = ws + z[cur]; q.lda = n.ldh[l];
    q.B = params + n.oW[l]; q.ldb = n.ld[l];
    q.M = B; q.N = n.in[l]; q.K = n.out[l];
    if (l > 0) {
      q.C = ws + z[cur ^ 1]; q.ldc = n.ldh[l - 1];
      q.dact = n.act; q.aux = ws + h[l - 1]; q.ldaux = n.ldh[l - 1];
    } else {
      q.C = ws + dx; q.ldc = ldsa;
    }
    gd.p[gd.nprob++] = q;
    const int rc = gm_gemm<false, true>(gd, st);
    if (rc != OSA_OK) return rc;
    cur ^= 1;
  }
  return OSA_OK;
}

// ---- clip_grad_norm_, the L2 term and Adam ---------------------------------------------------------------------------
// blockIdx.y = optimiser group: over its n contiguous floats, grad += 2 coeff w (ddpg.py:430-432) and the partial sums
// of grad^2 and w^2 of workgroup x into part[group][x][2]: a fixed assignment of elements to partials, added in order
// by the Adam launch.  Thread 0 of workgroup 0 advances the group's Adam step count.
struct TNorm {
  float* grad[2];
  const float* w[2];
  long n[2];
  int* adam_step[2];
  double* part;  // of the launch's first group
  float coeff;
};
__global__ __launch_bounds__(256) void td3_norm_kernel(TNorm g) {
  __shared__ double red[17];
  const int y = blockIdx.y;
  float* __restrict__ grad = y == 0 ? g.grad[0] : g.grad[1];
  const float* __restrict__ w = y == 0 ? g.w[0] : g.w[1];
  const long n = y == 0 ? g.n[0] : g.n[1];
  const float c2 = 2.f * g.coeff;
  double sg = 0.0, sw = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)T_NB * 256) {
    float gr = grad[e];
    if (g.coeff != 0.f) {
      const float x = w[e];
      gr = __fadd_rn(gr, __fmul_rn(c2, x));
      grad[e] = gr;
      sw += (double)x * x;
    }
    sg += (double)gr * gr;
  }
  sg = osa_block_sum<256>(sg, red);
  sw = osa_block_sum<256>(sw, red);
  if (threadIdx.x == 0) {
    g.part[((long)y * T_NB + blockIdx.x) * 2] = sg;
    g.part[((long)y * T_NB + blockIdx.x) * 2 + 1] = sw;
    if (blockIdx.x == 0) *(y == 0 ? g.adam_step[0] : g.adam_step[1]) += 1;
  }
}

// blockIdx.y = network; networks >= split belong to the launch's second group.  The clip scale from the group's
// partials, Adam, (target != null) the Polyak update; workgroup 0 of a group's first network writes its statistics.
struct TAdam {
  int Pn, split, B, nslots, kind;  // kind 0: critics (MSE rows + L2, mean q), 1: the actor (-mean q)
  long P, qstride;
  float *params, *m, *v, *target, *stats;
  const float *grad, *rows, *qtop;
  const double* part;
  const int* adam_step;  // [group]
  const long* step;
  float lr, max_norm, coeff, tau, omt;
  double beta1, beta2, eps;
};
__global__ __launch_bounds__(256) void td3_adam_kernel(TAdam g) {
  __shared__ double red[17];
  const int net = blockIdx.y, grp = net >= g.split ? 1 : 0;
  const double* part = g.part + (long)grp * T_NB * 2;
  double ng = 0.0, nw = 0.0;
  for (int i = 0; i < T_NB; ++i) {  // (every thread, the same order: no barrier needed for the scale itself)
    ng += part[2 * i];
    nw += part[2 * i + 1];
  }
  float scale = 1.f;
  if (g.max_norm > 0.f) scale = fminf(g.max_norm / ((float)sqrt(ng) + 1e-6f), 1.f);  // clip_grad_norm_
  if (blockIdx.x == 0 && (net == 0 || net == g.split)) {
    float* s = g.stats + (*g.step % g.nslots) * OSA_TD3_NSTAT;
    const int first = grp ? g.split : 0, nn = g.kind ? 1 : (grp ? 1 : g.split);
    const float* qtop = g.qtop + (long)first * g.qstride;
    double q = 0.0, l = 0.0;
    for (int b = threadIdx.x; b < g.B; b += 256) q += (double)qtop[4 * b];
    q = osa_block_sum<256>(q, red);
    float loss = 0.f;
    if (g.kind == 0) {
      for (int j = 0; j < nn; ++j) {  // mse_loss(q1, y) + mse_loss(q2, y): float32 means added in order
        l = 0.0;
        for (int b = threadIdx.x; b < g.B; b += 256) l += (double)g.rows[(long)(first + j) * g.B + b];
        l = osa_block_sum<256>(l, red);
        loss += (float)(l / g.B);
      }
      loss += (float)(nw * (double)g.coeff);
    }
    if (threadIdx.x == 0) {
      if (g.kind == 0) {
        s[grp ? 3 : 0] = loss;
        s[grp ? 4 : 1] = (float)(q / g.B);
      } else {
        s[2] = (float)(-q / g.B);
      }
    }
  }
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= g.Pn) return;
  const long o = (long)net * g.P + e;
  float mm = g.m[o], vv = g.v[o];
  const float w = crr_adam1(g.grad[o] * scale, mm, vv, g.params[o], g.lr, g.beta1, g.beta2, g.eps, g.adam_step[grp]);
  g.params[o] = w;
  g.m[o] = mm;
  g.v[o] = vv;
  if (g.target) g.target[o] = __fadd_rn(__fmul_rn(g.tau, w), __fmul_rn(g.omt, g.target[o]));
}

__global__ void td3_finish_kernel(long* step) {
  if (threadIdx.x == 0) *step += 1;
}

__device__ __forceinline__ float td3_normal(const uint32_t (&w)[4]) {  // as crr_draw_eps_kernel's
  const double u1 = (double)osa_u01(w[0]), u2 = (double)osa_u01(w[1]);
  return (float)(sqrt(-2.0 * log(u1)) * cos(6.28318530717958647692 * u2));
}

}  // namespace
