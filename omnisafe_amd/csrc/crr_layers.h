// What the offline actor-critic steps share (crr_kernels.hip: CRR / CCRR, bcq_kernels.hip: BCQ / BCQ-Lag): a network's
// padded block, its layer-wise forward and backward on the tile GEMM of gm_gemm.h, the normal draws and the Adam step
// with the Polyak update fused in.  Moved here unchanged from crr_kernels.hip; both translation units include it and get
// their own instantiations.
#pragma once
#include <math.h>

#include "gm_gemm.h"

namespace {

struct CNet {
  int L, in[GM_MAXL], out[GM_MAXL], ld[GM_MAXL], ldh[GM_MAXL], oW[GM_MAXL], ob[GM_MAXL];
  int oLS, Pn, P, act, maxldh;
};

inline int c4(int x) { return (x + 3) / 4 * 4; }

int crr_make_net(CNet& n, int in_dim, int L, const int* width, int act, int out_dim, bool log_std) {
  if (L < 2 || L > GM_MAXL) return OSA_EUNSUPPORTED;  // at least one hidden layer
  if (act < OSA_ACT_TANH || act > OSA_ACT_IDENTITY) return OSA_EUNSUPPORTED;
  n.L = L;
  n.act = act;
  n.maxldh = 4;
  int off = 0, prev = in_dim;
  for (int l = 0; l < L; ++l) {
    const int w = width[l];
    if (w < 1 || w > 4096) return OSA_EINVAL;
    n.in[l] = prev; n.out[l] = w; n.ld[l] = c4(prev); n.ldh[l] = c4(w);
    if (n.ldh[l] > n.maxldh) n.maxldh = n.ldh[l];
    n.oW[l] = off; off += w * n.ld[l];
    n.ob[l] = off; off += c4(w);
    prev = w;
  }
  if (prev != out_dim) return OSA_EINVAL;
  n.oLS = off;
  if (log_std) off += c4(out_dim);
  n.Pn = off;
  n.P = (off + 15) / 16 * 16;
  return OSA_OK;
}

GProb crr_prob() {
  GProb p = {};
  p.splits = 1;
  p.act = -1;
  p.dact = -1;
  p.ones_n = -1;
  return p;
}

// ---- layers ------------------------------------------------------------------------------------------------------
struct CFwd {
  const float* params;  // the network's parameter block
  const float* X;       // input rows
  int ldx, M;
  const size_t* h;      // workspace offsets of its layer outputs
};
// forward of up to four networks of one shape, layer by layer: up to three networks per launch
int crr_forward(const CNet& n, const CFwd* job, int njob, float* ws, hipStream_t st) {
  for (int l = 0; l < n.L; ++l)
    for (int j0 = 0; j0 < njob; j0 += (njob == 4 ? 2 : 3)) {
      GArgs g = {};
      g.splits = 1;
      const int j1 = j0 + (njob == 4 ? 2 : 3) < njob ? j0 + (njob == 4 ? 2 : 3) : njob;
      for (int j = j0; j < j1; ++j) {
        GProb p = crr_prob();
        p.A = l == 0 ? job[j].X : ws + job[j].h[l - 1];
        p.lda = l == 0 ? job[j].ldx : n.ldh[l - 1];
        p.B = job[j].params + n.oW[l];
        p.ldb = n.ld[l];
        p.C = ws + job[j].h[l];
        p.ldc = n.ldh[l];
        p.M = job[j].M; p.N = n.out[l]; p.K = n.in[l];
        p.bias = job[j].params + n.ob[l];
        p.act = l + 1 < n.L ? n.act : -1;
        g.p[g.nprob++] = p;
      }
      const int rc = gm_gemm<false, false>(g, st);
      if (rc != OSA_OK) return rc;
    }
  return OSA_OK;
}

struct CBwd {
  const float* params;
  const float* X;
  int ldx;
  const size_t* h;
  size_t z[2];  // ping-pong dL/d(pre-activation); z[0] holds the top layer's on entry
  float* grad;  // the network's gradient block (parameter layout)
};
// backward of up to two networks of one shape over B rows: dW_l (+ db_l) straight into the gradient block (one split:
// K = B rows), then dZ of the layer below
int crr_backward(const CNet& n, const CBwd* job, int njob, int B, float* ws, hipStream_t st) {
  int cur = 0;
  for (int l = n.L - 1; l >= 0; --l) {
    GArgs gw = {}, gd = {};
    gw.splits = 1;
    gd.splits = 1;
    for (int j = 0; j < njob; ++j) {
      GProb p = crr_prob();  // dW_l[out][in] (+ db_l) = dZ_l^T [out][rows] . {H_{l-1}, 1}[rows][in + 1]
      p.A = ws + job[j].z[cur]; p.lda = n.ldh[l];
      p.B = l == 0 ? job[j].X : ws + job[j].h[l - 1];
      p.ldb = l == 0 ? job[j].ldx : n.ldh[l - 1];
      p.C = job[j].grad + n.oW[l]; p.ldc = n.ld[l];
      p.cb = job[j].grad + n.ob[l]; p.cb_pad = c4(n.out[l]);
      p.M = n.out[l]; p.N = n.in[l]; p.K = B;
      p.ones_n = n.in[l];
      gw.p[gw.nprob++] = p;
      if (l > 0) {  // dZ_{l-1}[rows][in] = (dZ_l[rows][out] . W_l[out][in]) * act'(H_{l-1})
        GProb q = crr_prob();
        q.A = ws + job[j].z[cur]; q.lda = n.ldh[l];
        q.B = job[j].params + n.oW[l]; q.ldb = n.ld[l];
        q.C = ws + job[j].z[cur ^ 1]; q.ldc = n.ldh[l - 1];
        q.M = B; q.N = n.in[l]; q.K = n.out[l];
        q.dact = n.act; q.aux = ws + job[j].h[l - 1]; q.ldaux = n.ldh[l - 1];
        gd.p[gd.nprob++] = q;
      }
    }
    int rc;
    if ((rc = gm_gemm<true, true>(gw, st)) != OSA_OK) return rc;
    if (gd.nprob > 0 && (rc = gm_gemm<false, true>(gd, st)) != OSA_OK) return rc;
    cur ^= 1;
  }
  return OSA_OK;
}

// eps[slot][row][d]: the first Box-Muller normal of Philox(key, step, row A + d), key = seed ^ the buffer's constant
__global__ __launch_bounds__(256) void crr_draw_eps_kernel(unsigned long long key, long first, int nsteps, int nslots,
                                                           long per_step, float* __restrict__ eps) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)nsteps * per_step) return;
  const long k = e / per_step, i = e - k * per_step, step = first + k;
  uint32_t w[4];
  osa_philox(key, (uint64_t)step, (uint64_t)i, w);
  // osa_box_muller's first normal, evaluated in double and rounded once: a host restatement in float64 gives the same
  // float32 whatever the last bits of either side's log and cos (one launch per block of steps: off the step's path)
  const double u1 = (double)osa_u01(w[0]), u2 = (double)osa_u01(w[1]);
  eps[(step % nslots) * per_step + i] = (float)(sqrt(-2.0 * log(u1)) * cos(6.28318530717958647692 * u2));
}

// ---- (f) Adam (+ Polyak) -----------------------------------------------------------------------------------------
// torch.optim.Adam's step on one element: the factors 1 - beta are the float32 roundings of the DOUBLE differences, as
// torch forms them (1.f - 0.999f is off by 1.3e-5 of itself), the bias corrections are taken in double; IEEE sqrt and
// division.  t: the step count, this step included.
__device__ __forceinline__ float crr_adam1(float g, float& m, float& v, float w, float lr, double beta1, double beta2,
                                           double eps, int t) {
  const float b2 = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  m = fmaf(g - m, omb1, m);  // exp_avg.lerp_(grad, 1 - beta1)
  v = fmaf(g * g, omb2, v * b2);
  const float step_size = (float)((double)lr / (1.0 - pow(beta1, (double)t)));
  const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)t));
  const float denom = sqrtf(v) / bc2_sqrt + (float)eps;
  return w - step_size * (m / denom);
}

// blockIdx.y = network of the group; adam = 0: the Polyak update alone (a target whose network took no step)
__global__ __launch_bounds__(256) void crr_adam_kernel(int Pn, long P, float* __restrict__ params, float* __restrict__ m,
                                                       float* __restrict__ v, const float* __restrict__ grad,
                                                       long grad_stride, float* __restrict__ target,
                                                       const int* __restrict__ adam_step, int adam, float lr,
                                                       double beta1, double beta2, double eps, float tau,
                                                       float one_minus_tau) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Pn) return;
  const long o = (long)blockIdx.y * P + e;
  float w = params[o];
  if (adam) {
    float mm = m[o], vv = v[o];
    w = crr_adam1(grad[(long)blockIdx.y * grad_stride + e], mm, vv, w, lr, beta1, beta2, eps, *adam_step);
    params[o] = w;
    m[o] = mm;
    v[o] = vv;
  }
  if (target) target[o] = __fadd_rn(__fmul_rn(tau, w), __fmul_rn(one_minus_tau, target[o]));
}

unsigned crr_blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
