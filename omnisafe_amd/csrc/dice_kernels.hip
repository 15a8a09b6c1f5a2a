// Offline COptiDICE trained on the device from a device-resident dataset: omnisafe/algorithms/offline/coptidice.py:162-290
// with the ObsEncoder networks nu and chi of models/offline/dice.py:27-87 and a gaussian_learning actor.
//
// At the YAML shape (batch 256, hidden 256 x 256 x 256) a layer is a 768 x 256 x 256 product: microseconds of arithmetic,
// and a step of layer-wise launches is bound by how many launches it takes.  So the layer kernel here takes a LIST of
// independent GEMM problems per launch (dice_list_kernel), and a step makes one launch per layer DEPTH:
//   * the tile is vae_skinny_kernel's: one workgroup per 32 x 32 float32-MFMA output tile, the tile's K range split over
//     the four waves in whole 32-wide chunks, each wave staging its own chunk of either operand through a wave-private
//     LDS panel with the next chunk's global loads in flight, the four partial tiles added in LDS in wave order 0, 1, 2,
//     3 (fixed order: bit-reproducible), every wave finishing a quarter of the tile's rows;
//   * the grid is ONE dimension: a prefix table maps the workgroup id to (problem, tile) -- problems of different sizes
//     pad nothing, a network contributes no problem at a depth it does not have;
//   * every problem carries its own operands (rows gathered through idx[slot] from up to three dataset arrays laid end to
//     end: obs[idx] || next_obs[idx] || init_obs[idx] is never copied), transposes, bias / activation / activation'
//     epilogue and bias-gradient column.
// Per step: nu and chi forward over 3 B rows (one launch per hidden depth), the heads-and-losses kernel (one workgroup:
// the N = 1 heads as row dots, the row math, the batch reductions, both heads' gradients, the Adam steps of lambda and
// tau), the backward of both networks (dZ and dW of both: four problems a launch), one Adam launch over nu and chi, the nu
// re-forward over 2 B rows together with the actor's forward over B rows, the policy kernel (nu head, w, the weighted
// log-likelihood and its gradient), the actor's backward, its Adam, and the finish (PolicyStd, step counter).
// OSA_DICE_ROUTE_SINGLE launches every problem alone (the comparison of tools/dice_timing.py).
// All stores are plain vector stores; no atomics, no cooperative launch.
#include <math.h>

#include "crr_layers.h"

namespace {

constexpr int DL_MAXP = 8;     // problems of a launch
constexpr int DL_T = 32;       // tile edge = the MFMA's, and the K chunk of a stage
constexpr int DL_LD = DL_T + 4;
constexpr int DH_THREADS = 1024;
constexpr int DICE_MAX_B = 1024;  // one thread per batch row in the heads kernel; 2 x 3 B outputs in its LDS

struct DLayout {
  CNet n[3];  // nu, chi, actor
  int D, A, B, fn, lda;
};

int dice_make_layout(const osa_dice_desc* d, DLayout* lo) {
  if (!d) return OSA_EINVAL;
  if (d->obs_dim < 1 || d->obs_dim > 4096 || d->act_dim < 1 || d->act_dim > 64 || d->batch < 1) return OSA_EINVAL;
  if (d->fn_type < OSA_DICE_FN_KL || d->fn_type > OSA_DICE_FN_CHISQUARE) return OSA_EUNSUPPORTED;
  if (d->batch > DICE_MAX_B) return OSA_EUNSUPPORTED;
  lo->D = d->obs_dim; lo->A = d->act_dim; lo->B = d->batch; lo->fn = d->fn_type; lo->lda = c4(lo->A);
  for (int k = 0; k < 3; ++k) {
    const int nh = d->n_hidden[k];
    if (nh < 1 || nh + 1 > GM_MAXL) return OSA_EUNSUPPORTED;
    int width[GM_MAXL];
    for (int l = 0; l < nh; ++l) width[l] = d->hidden[k][l];
    width[nh] = k == 2 ? lo->A : 1;
    const int rc = crr_make_net(lo->n[k], lo->D, nh + 1, width, d->activation[k], width[nh], k == 2);
    if (rc != OSA_OK) return rc;
  }
  return OSA_OK;
}

struct DWs {
  size_t h[3][GM_MAXL], z[3][2], dout[2], w, grad[3], total;
};
DWs dice_ws(const DLayout& lo) {
  DWs w = {};
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 3) / 4 * 4;
    return o;
  };
  for (int k = 0; k < 3; ++k) {
    const size_t rows = k == 2 ? lo.B : 3 * (size_t)lo.B;
    for (int l = 0; l < lo.n[k].L; ++l) w.h[k][l] = take(rows * lo.n[k].ldh[l]);
    for (int q = 0; q < 2; ++q) w.z[k][q] = take(rows * lo.n[k].maxldh);
    w.grad[k] = take(lo.n[k].P);
  }
  for (int q = 0; q < 2; ++q) w.dout[q] = take(3 * (size_t)lo.B);
  w.w = take(lo.B);
  w.total = off;
  return w;
}

// ---- the problem-list layer kernel -------------------------------------------------------------------------------
// An operand as it lies in memory: rows of `ld` floats.  seg > 0: memory row r is row idx[r % seg] of dataset array
// p[r / seg] (up to three arrays laid end to end).  vec: 16-byte loads are safe (plain rows, aligned base, ld % 4 == 0).
struct DSrc {
  const float* p[3];
  int ld[3], seg, vec;
};
// C[m][n] = epi(sum_k A(m, k) B(k, n)).  at: A(m, k) = A[k][m] (else A[m][k]); bt: B(k, n) = B[k][n] (else B[n][k]).
// Epilogue: + bias[n], activation, * act'(aux[m][n]); ones_n >= 0 (with bt): B(k, ones_n) = 1, that column of the product
// goes to cb[m] (the bias gradient), cb[M .. cb_pad) and C[m][N .. ldc) are written zero.  tx: column tiles.
struct DProb {
  DSrc A, Bm;
  float* C;
  const float* bias;
  const float* aux;
  float* cb;
  int at, bt, M, N, K, ldc, ldaux, act, dact, ones_n, cb_pad, tx;
};
struct DArgs {
  DProb p[DL_MAXP];
  int tile0[DL_MAXP + 1];  // workgroup b serves tile b - tile0[y] of problem y, tile0[y] <= b < tile0[y + 1]
  int nprob;
  const long* idx;         // [nslots][B]
  const long* step;
  int nslots, B;
  long nrows;
};

__device__ __forceinline__ f32x4 dl_fetch(const DSrc& s, const long* __restrict__ idx, long nrows, int mr, int mc, int lim,
                                          bool ok) {
  if (s.vec) return gm_load4(s.p[0] + (long)mr * s.ld[0], mc, lim, ok);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!ok || mc >= lim) return v;
  const float* row;
  if (s.seg) {
    const int sg = mr / s.seg;  // (ok: mr is a row of the problem, sg < the arrays it names)
    long g = idx[mr - sg * s.seg];
    if (g < 0 || g >= nrows) g = 0;  // (injected indices are checked on the host; never read outside the dataset)
    row = (sg == 0 ? s.p[0] : (sg == 1 ? s.p[1] : s.p[2])) + g * (sg == 0 ? s.ld[0] : (sg == 1 ? s.ld[1] : s.ld[2]));
  } else {
    row = s.p[0] + (long)mr * s.ld[0];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (mc + i < lim) v[i] = row[mc + i];
  return v;
}

__global__ __launch_bounds__(256) void dice_list_kernel(DArgs g) {
  // [wave][A panel | B panel]; after the K loop the first 4 x 16 x 64 floats hold the four partial tiles
  __shared__ __attribute__((aligned(16))) float smem[4 * 2 * DL_T * DL_LD];
  // the prefix table: selected with scalar compares (a run-time index into the by-value argument would go through scratch)
  int y = 0;
#pragma unroll
  for (int q = 1; q < DL_MAXP; ++q)
    if (q < g.nprob && (int)blockIdx.x >= g.tile0[q]) y = q;
  DProb p = g.p[0];
  int t0 = g.tile0[0];
#pragma unroll
  for (int q = 1; q < DL_MAXP; ++q)
    if (q == y) { p = g.p[q]; t0 = g.tile0[q]; }
  const int tile = blockIdx.x - t0;
  const int M = p.M, N = p.N, K = p.K;
  const int m0 = (tile / p.tx) * DL_T, n0 = (tile % p.tx) * DL_T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
  const long* __restrict__ idx = g.idx ? g.idx + (*g.step % g.nslots) * g.B : nullptr;  // (null: no gathered operand)
  // this wave's quarter of K in whole chunks; every wave runs the same number of stages (the barriers are uniform)
  const int nst = (K + 4 * DL_T - 1) / (4 * DL_T);
  const int kbeg = wave * nst * DL_T;
  const int kend = K < kbeg + nst * DL_T ? K : kbeg + nst * DL_T;
  float* sA = smem + wave * 2 * DL_T * DL_LD;
  float* sB = sA + DL_T * DL_LD;
  f32x4 ra[4], rb[4];
  auto load_chunk = [&](int s) {
    const int k0 = kbeg + s * DL_T;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = lane + 64 * q, hi = u >> 3, c = 4 * (u & 7);
      // at: memory row = k, 32 consecutive m; else memory row = m, 32 consecutive k
      ra[q] = p.at ? dl_fetch(p.A, idx, g.nrows, k0 + hi, m0 + c, M, k0 + hi < kend)
                   : dl_fetch(p.A, idx, g.nrows, m0 + hi, k0 + c, kend, m0 + hi < M);
      if (p.bt) {
        f32x4 v = dl_fetch(p.Bm, idx, g.nrows, k0 + hi, n0 + c, N, k0 + hi < kend);
        if (p.ones_n >= 0 && k0 + hi < kend) {  // the column of ones: the bias gradient is one more output column
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (n0 + c + i == p.ones_n) v[i] = 1.f;
        }
        rb[q] = v;
      } else {
        rb[q] = dl_fetch(p.Bm, idx, g.nrows, n0 + hi, k0 + c, kend, n0 + hi < N);
      }
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = lane + 64 * q, hi = u >> 3, c = 4 * (u & 7);
      if (p.at) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sA[(c + i) * DL_LD + hi] = ra[q][i];
      } else {
        *reinterpret_cast<f32x4*>(&sA[hi * DL_LD + c]) = ra[q];
      }
      if (p.bt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sB[(c + i) * DL_LD + hi] = rb[q][i];
      } else {
        *reinterpret_cast<f32x4*>(&sB[hi * DL_LD + c]) = rb[q];
      }
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (kbeg < kend) load_chunk(0);
  for (int s = 0; s < nst; ++s) {
    const bool live = kbeg + s * DL_T < kend;  // wave-uniform
    __syncthreads();                            // the panels' last readers are done
    if (live) store_chunk();
    __syncthreads();
    if (kbeg + (s + 1) * DL_T < kend && s + 1 < nst) load_chunk(s + 1);  // in flight under this chunk's MFMAs
    if (live) {
#pragma unroll
      for (int j = 0; j < DL_T / 8; ++j) {
        // lane group kk consumes k = 8 j + 4 kk + q in MFMA step q, for A and B alike
        const f32x4 af = *reinterpret_cast<const f32x4*>(&sA[l31 * DL_LD + 8 * j + 4 * kk]);
        const f32x4 bf = *reinterpret_cast<const f32x4*>(&sB[l31 * DL_LD + 8 * j + 4 * kk]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q], bf[q], acc, 0, 0, 0);
      }
    }
  }
  // ---- the ordered reduce: partial tile of wave w at smem[w][r][lane]
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) smem[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();
  const int n = n0 + l31;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 4 * wave + i;
    float v = smem[(0 * 16 + r) * 64 + lane];
    v += smem[(1 * 16 + r) * 64 + lane];
    v += smem[(2 * 16 + r) * 64 + lane];
    v += smem[(3 * 16 + r) * 64 + lane];
    const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kk;  // D[row][col = l31] of the 32 x 32 MFMA
    if (m < M) {
      if (n < N) {
        if (p.bias) v += p.bias[n];
        if (p.act >= 0) v = gm_act(v, p.act);
        if (p.dact >= 0) v *= gm_dact(p.aux[(long)m * p.ldaux + n], p.dact);
        p.C[(long)m * p.ldc + n] = v;
      } else {
        if (n == p.ones_n && p.cb) p.cb[m] = v;
        if (n < p.ldc) p.C[(long)m * p.ldc + n] = 0.f;  // padding columns of the row
      }
    } else if (n == p.ones_n && p.cb && m < p.cb_pad) {
      p.cb[m] = 0.f;  // padding of the bias block
    }
  }
}

DSrc dl_plain(const float* p, int ld) {
  DSrc s = {};
  s.p[0] = p;
  s.ld[0] = ld;
  s.vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0;
  return s;
}
DProb dl_prob() {
  DProb p = {};
  p.act = -1;
  p.dact = -1;
  p.ones_n = -1;
  return p;
}

struct DCtx {  // what every launch of a step shares
  const long* idx;
  const long* step;
  int nslots, B;
  long nrows;
  bool single;  // every problem in a launch of its own
  hipStream_t st;
};

int dl_launch(const DCtx& c, const DProb* p, int n) {
  for (int i0 = 0; i0 < n; i0 += c.single ? 1 : DL_MAXP) {
    const int i1 = c.single ? i0 + 1 : (i0 + DL_MAXP < n ? i0 + DL_MAXP : n);
    DArgs g = {};
    int tiles = 0;
    for (int i = i0; i < i1; ++i) {
      DProb q = p[i];
      const int nc = q.ldc > q.N + (q.ones_n >= 0 ? 1 : 0) ? q.ldc : q.N + (q.ones_n >= 0 ? 1 : 0);
      q.tx = (nc + DL_T - 1) / DL_T;
      g.tile0[g.nprob] = tiles;
      g.p[g.nprob++] = q;
      tiles += q.tx * ((q.M + DL_T - 1) / DL_T);
    }
    for (int i = g.nprob; i <= DL_MAXP; ++i) g.tile0[i] = tiles;
    if (tiles == 0) continue;
    g.idx = c.idx; g.step = c.step; g.nslots = c.nslots; g.B = c.B; g.nrows = c.nrows;
    hipLaunchKernelGGL(dice_list_kernel, dim3(tiles), dim3(256), 0, c.st, g);
    if (hipGetLastError() != hipSuccess) return OSA_EHIP;
  }
  return OSA_OK;
}

// one network's part in the per-depth launches
struct DNetJob {
  const CNet* n;
  const float* params;
  DSrc x0;            // the first layer's input rows
  int M;              // rows
  float* const* h;    // layer outputs
  float* const* z;    // ping-pong dL/d(pre-activation); z[0] holds the top layer's on entry of the backward
  float* grad;
  int top;            // forward: linear layers that run on the list kernel (the N = 1 heads do not)
};

// forward, one launch per depth: layer l of every network that has one
int dice_forward(const DCtx& c, const DNetJob* job, int njob) {
  int depth = 0;
  for (int j = 0; j < njob; ++j) depth = job[j].top > depth ? job[j].top : depth;
  for (int l = 0; l < depth; ++l) {
    DProb p[DL_MAXP];
    int np = 0;
    for (int j = 0; j < njob; ++j) {
      const CNet& n = *job[j].n;
      if (l >= job[j].top) continue;
      DProb& q = p[np++] = dl_prob();
      q.A = l == 0 ? job[j].x0 : dl_plain(job[j].h[l - 1], n.ldh[l - 1]);
      q.Bm = dl_plain(job[j].params + n.oW[l], n.ld[l]);
      q.C = job[j].h[l]; q.ldc = n.ldh[l];
      q.M = job[j].M; q.N = n.out[l]; q.K = n.in[l];
      q.bias = job[j].params + n.ob[l];
      q.act = l + 1 < n.L ? n.act : -1;
    }
    const int rc = dl_launch(c, p, np);
    if (rc != OSA_OK) return rc;
  }
  return OSA_OK;
}

// backward, one launch per distance from the top: dW + db straight into the gradient block and dZ of the layer below,
// which read the same dZ and leave together
int dice_backward(const DCtx& c, const DNetJob* job, int njob) {
  int depth = 0;
  for (int j = 0; j < njob; ++j) depth = job[j].n->L > depth ? job[j].n->L : depth;
  for (int t = 0; t < depth; ++t) {
    DProb p[DL_MAXP];
    int np = 0;
    for (int j = 0; j < njob; ++j) {
      const CNet& n = *job[j].n;
      const int l = n.L - 1 - t, cur = t & 1;
      if (l < 0) continue;
      {  // dW_l[out][in] (+ db_l) = dZ_l^T [out][rows] . {H_{l-1}, 1}[rows][in + 1]
        DProb& q = p[np++] = dl_prob();
        q.at = 1; q.bt = 1;
        q.A = dl_plain(job[j].z[cur], n.ldh[l]);
        q.Bm = l == 0 ? job[j].x0 : dl_plain(job[j].h[l - 1], n.ldh[l - 1]);
        q.C = job[j].grad + n.oW[l]; q.ldc = n.ld[l];
        q.cb = job[j].grad + n.ob[l]; q.cb_pad = c4(n.out[l]);
        q.M = n.out[l]; q.N = n.in[l]; q.K = job[j].M;
        q.ones_n = n.in[l];
      }
      if (l > 0) {  // dZ_{l-1}[rows][in] = (dZ_l[rows][out] . W_l[out][in]) * act'(H_{l-1})
        DProb& q = p[np++] = dl_prob();
        q.bt = 1;
        q.A = dl_plain(job[j].z[cur], n.ldh[l]);
        q.Bm = dl_plain(job[j].params + n.oW[l], n.ld[l]);
        q.C = job[j].z[cur ^ 1]; q.ldc = n.ldh[l - 1];
        q.M = job[j].M; q.N = n.in[l]; q.K = n.out[l];
        q.dact = n.act; q.aux = job[j].h[l - 1]; q.ldaux = n.ldh[l - 1];
      }
    }
    const int rc = dl_launch(c, p, np);
    if (rc != OSA_OK) return rc;
  }
  return OSA_OK;
}

// ---- draws -------------------------------------------------------------------------------------------------------
#define DICE_KEY_IDX 0x44494345494458ull /* a key of its own: seed ^ key, counter = (step, element) */

// idx[slot][b]: 64 random bits, multiply-high into [0, N)
__global__ __launch_bounds__(256) void dice_draw_idx_kernel(unsigned long long seed, long first, int nsteps, int nslots,
                                                            int B, unsigned long long N, long* __restrict__ idx) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)nsteps * B) return;
  const long k = e / B, b = e - k * B, step = first + k;
  uint32_t w[4];
  osa_philox(seed ^ DICE_KEY_IDX, (uint64_t)step, (uint64_t)b, w);
  const unsigned long long bits = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
  idx[(step % nslots) * B + b] = (long)__umul64hi(bits, N);
}

// ---- heads -------------------------------------------------------------------------------------------------------
// out[r] = <h[r][0 .. K), w> + b of rows r0 + wave, r0 + wave + 16, ...: one wave per row, the lanes stride the columns,
// the wave sum in the shuffle tree's fixed order
__device__ __forceinline__ void dice_row_dots(const float* __restrict__ h, int ldh, int K, const float* __restrict__ w,
                                              float b, int rows, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < rows; r += DH_THREADS / 64) {
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s = fmaf(h[(long)r * ldh + k], w[k], s);
    s = osa_wave_sum(s);
    if (lane == 0) out[r] = s + b;
  }
}

// w = relu(f_inv(adv / alpha)) and dw/dadv (coptidice.py:292-323)
__device__ __forceinline__ float dice_w(int fn, float adv, float alpha, float* dw) {
  const float x = adv / alpha;
  float y, dy;
  if (fn == OSA_DICE_FN_KL) {
    y = expf(x - 1.f); dy = y;
  } else if (fn == OSA_DICE_FN_SOFTCHI) {
    if (x < 0.f) { y = expf(fminf(x, 0.f)); dy = y; } else { y = x + 1.f; dy = 1.f; }
  } else {
    y = x + 1.f; dy = 1.f;
  }
  *dw = y > 0.f ? dy / alpha : 0.f;
  return fmaxf(y, 0.f);
}
// f(w) and f'(w)
__device__ __forceinline__ float dice_f(int fn, float w, float* df) {
  const float lg = logf(w + 1e-10f);
  if (fn == OSA_DICE_FN_KL) { *df = lg + w / (w + 1e-10f); return w * lg; }
  if (fn == OSA_DICE_FN_SOFTCHI && w < 1.f) { *df = (lg - 1.f) + w / (w + 1e-10f); return w * (lg - 1.f) + 1.f; }
  *df = w - 1.f;
  return 0.5f * (w - 1.f) * (w - 1.f);
}

// scalar Adam of a multiplier {value, m, v}, then the clamp
__device__ __forceinline__ float dice_scalar_adam(float* s, float grad, float lr, double b1, double b2, double eps, int t,
                                                  float lo, float hi) {
  float m = s[1], v = s[2];
  float x = crr_adam1(grad, m, v, s[0], lr, b1, b2, eps, t);
  x = fminf(fmaxf(x, lo), hi);
  s[0] = x; s[1] = m; s[2] = v;
  return x;
}

// deterministic sum of a [rows] column times the rows of h, per column k: the threads form groups of CW columns, group g
// walks rows g, g + G, ...; the groups' partials meet in LDS and are added in group order.  out[k] for k < ldw (zero from
// K on); returns nothing.  part: DH_THREADS floats.
__device__ __forceinline__ void dice_head_grad(const float* __restrict__ h, int ldh, int K, int ldw, const float* d, int rows,
                                               float* part, float* __restrict__ out) {
  const int CW = K >= DH_THREADS ? DH_THREADS : (K + 63) / 64 * 64, G = DH_THREADS / CW;
  const int col = threadIdx.x % CW, grp = threadIdx.x / CW;
  for (int c0 = 0; c0 < ldw; c0 += CW) {
    const int k = c0 + col;
    float s = 0.f;
    if (grp < G && k < K)
      for (int r = grp; r < rows; r += G) s = fmaf(d[r], h[(long)r * ldh + k], s);
    __syncthreads();
    part[threadIdx.x] = s;
    __syncthreads();
    if (grp == 0 && k < ldw) {
      float v = 0.f;
      for (int q = 0; q < G; ++q) v += part[q * CW + col];
      out[k] = k < K ? v : 0.f;
    }
  }
}

struct DHead {
  const float *h[2], *w[2], *b[2];  // last hidden rows [3 B][ldh], head weights and bias of nu, chi
  int K[2], ldh[2], ldw[2];
  const float *reward, *cost, *done;
  const long* idx;
  const long* step;
  long nrows;
  int nslots, B, fn;
  float gamma, alpha, cost_limit, cost_ub_eps, lr_lamb, lr_tau;
  double beta1, beta2, eps;
  float* mult;      // [8]: lambda, m, v, -, tau, m, v, -
  int* adam_step;   // [0]: nu, chi, lambda, tau
  float* dout[2];   // [3 B] dL/d(output) of nu, chi
  float *gw[2], *gb[2];
  float* stats;
};
// coptidice.py:184-246 behind the last hidden layers, one workgroup
__global__ __launch_bounds__(DH_THREADS) void dice_heads_kernel(DHead g) {
  __shared__ float s_out[2][3 * DICE_MAX_B];
  __shared__ float part[DH_THREADS];
  __shared__ double red[17];
  __shared__ float s_max[DH_THREADS / 64];
  const int tid = threadIdx.x, B = g.B, lane = tid & 63, wave = tid >> 6;
  const long slot = *g.step % g.nslots;
  for (int k = 0; k < 2; ++k) dice_row_dots(g.h[k], g.ldh[k], g.K[k], g.w[k], g.b[k][0], 3 * B, s_out[k]);
  __syncthreads();
  const float lam = g.mult[0], tau = g.mult[4], invB = 1.f / (float)B, omg = 1.f - g.gamma;
  const bool on = tid < B;
  float c = 0.f, nd = 0.f, adv = 0.f, w = 0.f, dw = 0.f, fw = 0.f, df = 0.f, ell = 0.f, e = 0.f;
  if (on) {
    long i = g.idx[slot * B + tid];
    if (i < 0 || i >= g.nrows) i = 0;
    c = g.cost[i];
    nd = 1.f - g.done[i];
    adv = g.reward[i] - lam * c + nd * g.gamma * s_out[0][B + tid] - s_out[0][tid];
    w = dice_w(g.fn, adv, g.alpha, &dw);
    fw = dice_f(g.fn, w, &df);
    e = c + g.gamma * nd * s_out[1][B + tid] - s_out[1][tid];
    ell = omg * s_out[1][2 * B + tid] + w * e;
  }
  const double s_init = osa_block_sum<DH_THREADS>(on ? (double)s_out[0][2 * B + tid] : 0.0, red);
  const double s_f = osa_block_sum<DH_THREADS>((double)fw, red);
  const double s_wadv = osa_block_sum<DH_THREADS>((double)(w * adv), red);
  const double s_wc = osa_block_sum<DH_THREADS>((double)(w * c), red);
  // softmax over the batch of ell / tau with max-subtraction
  const float logit = ell / tau;
  const float wm = osa_wave_max(on ? logit : -INFINITY);
  if (lane == 0) s_max[wave] = wm;
  __syncthreads();
  float mx = s_max[0];
  for (int q = 1; q < DH_THREADS / 64; ++q) mx = fmaxf(mx, s_max[q]);
  const float ex = on ? expf(logit - mx) : 0.f;
  const float zsum = (float)osa_block_sum<DH_THREADS>((double)ex, red);
  const float pj = ex / zsum, wt = pj * (float)B;
  const float lw = on ? (logit - mx) - logf(zsum) + logf((float)B) : 0.f;
  const double s_pl = osa_block_sum<DH_THREADS>((double)(pj * ell), red);
  const double s_kl = osa_block_sum<DH_THREADS>(on ? (double)(wt * lw - wt + 1.f) : 0.0, red);
  const float kl = (float)(s_kl / B), cost_ub = (float)(s_wc / B), chi_loss = (float)s_pl;
  __syncthreads();  // (every s_out read above is done)
  if (on) {
    // d nu_loss / d adv = (w + dw (adv - alpha f'(w))) / B;  d chi_loss / d ell = p (1 + (ell - sum p ell) / tau)
    const float da = (w + dw * (adv - g.alpha * df)) * invB;
    s_out[0][tid] = -da;
    s_out[0][B + tid] = nd * g.gamma * da;
    s_out[0][2 * B + tid] = omg * invB;
    const float ge = pj * (1.f + (ell - chi_loss) / tau);
    s_out[1][tid] = -(w * ge);
    s_out[1][B + tid] = g.gamma * nd * w * ge;
    s_out[1][2 * B + tid] = omg * ge;
  }
  __syncthreads();
  for (int k = 0; k < 2; ++k) {
    for (int r = tid; r < 3 * B; r += DH_THREADS) g.dout[k][r] = s_out[k][r];
    dice_head_grad(g.h[k], g.ldh[k], g.K[k], g.ldw[k], s_out[k], 3 * B, part, g.gw[k]);
    const double sb = osa_block_sum<DH_THREADS>(tid < B ? (double)s_out[k][tid] + (double)s_out[k][B + tid] +
                                                              (double)s_out[k][2 * B + tid] : 0.0, red);
    if (tid < 4) g.gb[k][tid] = tid == 0 ? (float)sb : 0.f;
  }
  if (tid == 0) {
    const int t = *g.adam_step + 1;
    *g.adam_step = t;
    float* s = g.stats + slot * OSA_DICE_NSTAT;
    s[0] = (float)(omg * (s_init / B) - g.alpha * (s_f / B) + s_wadv / B);
    s[1] = chi_loss;
    s[2] = -(lam * (cost_ub - g.cost_limit));
    s[3] = -tau * (kl - g.cost_ub_eps);
    s[4] = cost_ub;
    s[5] = kl;
    s[7] = dice_scalar_adam(g.mult, -(cost_ub - g.cost_limit), g.lr_lamb, g.beta1, g.beta2, g.eps, t, 0.f, 1e3f);
    s[6] = dice_scalar_adam(g.mult + 4, -(kl - g.cost_ub_eps), g.lr_tau, g.beta1, g.beta2, g.eps, t, 1e-6f, INFINITY);
    s[10] = 0.f;
    s[11] = 0.f;
  }
}

struct DPolicy {
  const float *h, *wv, *bv;  // nu's last hidden rows [2 B][ldh] with the UPDATED weights, its head
  int K, ldh;
  const float *reward, *cost, *done, *act;
  int ld_act;
  const long* idx;
  const long* step;
  long nrows;
  int nslots, B, A, lda, fn;
  float gamma, alpha;
  const float* mult;     // [0]: the UPDATED lambda
  const float *mu, *log_std;
  float *w, *dz, *g_log_std, *stats;
  int* adam_step;        // the actor's
};
// coptidice.py:257-265: w from the updated nu and lambda, -(w logp(action)).mean() and its gradient
__global__ __launch_bounds__(DH_THREADS) void dice_policy_kernel(DPolicy g) {
  __shared__ float s_nu[2 * DICE_MAX_B];
  __shared__ double red[17];
  const int tid = threadIdx.x, B = g.B;
  const long slot = *g.step % g.nslots;
  dice_row_dots(g.h, g.ldh, g.K, g.wv, g.bv[0], 2 * B, s_nu);
  __syncthreads();
  const bool on = tid < B;
  const float invB = 1.f / (float)B;
  float w = 0.f, lp = 0.f;
  long i = 0;
  if (on) {
    i = g.idx[slot * B + tid];
    if (i < 0 || i >= g.nrows) i = 0;
    float dw;
    const float adv = g.reward[i] - g.mult[0] * g.cost[i] + (1.f - g.done[i]) * g.gamma * s_nu[B + tid] - s_nu[tid];
    w = dice_w(g.fn, adv, g.alpha, &dw);
    g.w[tid] = w;
  }
  for (int d = 0; d < g.lda; ++d) {
    double gl = 0.0;
    if (on) {
      float dz = 0.f;
      if (d < g.A) {
        const float sd = expf(g.log_std[d]), var = sd * sd;
        const float diff = g.act[i * g.ld_act + d] - g.mu[(long)tid * g.lda + d];
        lp += -(diff * diff) / (2.f * var) - logf(sd) - 0.91893853320467274178f;
        dz = -(w * invB) * diff / var;
        gl = (double)(w * invB) * (1.0 - (double)(diff * diff / var));
      }
      g.dz[(long)tid * g.lda + d] = dz;
    }
    gl = osa_block_sum<DH_THREADS>(gl, red);  // (block-uniform loop: every thread calls)
    if (tid == 0) g.g_log_std[d] = (float)gl;
  }
  const double loss = osa_block_sum<DH_THREADS>((double)w * (double)(-lp), red);
  if (tid == 0) {
    g.stats[slot * OSA_DICE_NSTAT + 8] = (float)(loss / B);
    *g.adam_step += 1;
  }
}

// ---- Adam --------------------------------------------------------------------------------------------------------
struct DAdam {
  float *params[2], *m[2], *v[2];
  const float* grad[2];
  int Pn[2];
  float lr[2];
  const int* adam_step[2];
  double beta1, beta2, eps;
};
// blockIdx.y = network; torch.optim.Adam's step (crr_adam1), each network at its own learning rate
__global__ __launch_bounds__(256) void dice_adam_kernel(DAdam g) {
  const int k = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= g.Pn[k]) return;
  float mm = g.m[k][e], vv = g.v[k][e];
  g.params[k][e] = crr_adam1(g.grad[k][e], mm, vv, g.params[k][e], g.lr[k], g.beta1, g.beta2, g.eps, *g.adam_step[k]);
  g.m[k][e] = mm;
  g.v[k][e] = vv;
}

// the step's last launch: PolicyStd of the UPDATED actor (coptidice.py:273), then the step counter advances -- nothing
// after this reads the step's slot
__global__ void dice_finish_kernel(const float* __restrict__ log_std, int A, float* __restrict__ stats, long* step,
                                   int nslots) {
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int d = 0; d < A; ++d) sum += (double)expf(log_std[d]);
  stats[(*step % nslots) * OSA_DICE_NSTAT + 9] = (float)(sum / A);
  *step += 1;
}

// out[r] of plain rows (osa_dice_values)
__global__ __launch_bounds__(DH_THREADS) void dice_dots_kernel(const float* h, int ldh, int K, const float* w,
                                                               const float* b, int rows, float* out) {
  dice_row_dots(h, ldh, K, w, b[0], rows, out);
}

// dataset rows through idx: obs[idx] || next_obs[idx] || init_obs[idx], B rows each
DSrc dice_gather(const osa_dice_data* d, int B) {
  DSrc s = {};
  s.p[0] = d->obs; s.ld[0] = d->ld_obs;
  s.p[1] = d->next_obs; s.ld[1] = d->ld_next;
  s.p[2] = d->init_obs; s.ld[2] = d->ld_init;
  s.seg = B;
  return s;
}

}  // namespace

extern "C" {

int osa_dice_layout(const osa_dice_desc* desc, int* out) {
  DLayout lo;
  OSA_REQUIRE(desc && out);
  const int rc = dice_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  out[0] = lo.n[0].P; out[1] = lo.n[1].P; out[2] = lo.n[2].P; out[3] = lo.n[2].oLS; out[4] = OSA_DICE_NSTAT;
  out[5] = DICE_MAX_B;
  int k = 6;
  for (int net = 0; net < 3; ++net)
    for (int l = 0; l < OSA_GMLP_MAX_LAYERS; ++l) {
      const CNet& n = lo.n[net];
      out[k++] = l < n.L ? n.oW[l] : -1;
      out[k++] = l < n.L ? n.ob[l] : -1;
      out[k++] = l < n.L ? n.ld[l] : 0;
    }
  return OSA_OK;
}

size_t osa_dice_ws_floats(const osa_dice_desc* desc) {
  DLayout lo;
  if (dice_make_layout(desc, &lo) != OSA_OK) return 0;
  return dice_ws(lo).total;
}

int osa_dice_draws(const osa_dice_desc* desc, unsigned long long seed, long first_step, int nsteps, int nslots,
                   long n_rows, long* idx, void* stream) {
  DLayout lo;
  OSA_REQUIRE(desc && idx);
  const int rc = dice_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(first_step >= 0 && nsteps >= 1 && nslots >= 1 && nsteps <= nslots && n_rows >= 1);
  hipLaunchKernelGGL(dice_draw_idx_kernel, dim3(crr_blocks((long)nsteps * lo.B, 256)), dim3(256), 0, osa_stream(stream),
                     seed, first_step, nsteps, nslots, lo.B, (unsigned long long)n_rows, idx);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

int osa_dice_step(const osa_dice_desc* desc, const osa_dice_hparams* hp, const osa_dice_state* s,
                  const osa_dice_data* data, const osa_dice_draw_buffers* dr, float* stats, float* ws, size_t ws_floats,
                  int nsteps, void* stream) {
  DLayout lo;
  OSA_REQUIRE(desc && hp && s && data && dr && stats && ws && nsteps >= 1);
  const int rc0 = dice_make_layout(desc, &lo);
  if (rc0 != OSA_OK) return rc0;
  OSA_REQUIRE(hp->route == OSA_DICE_ROUTE_LIST || hp->route == OSA_DICE_ROUTE_SINGLE);
  const DWs w = dice_ws(lo);
  OSA_REQUIRE(ws_floats >= w.total && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  OSA_REQUIRE(s->nu && s->nu_m && s->nu_v && s->chi && s->chi_m && s->chi_v && s->actor && s->actor_m && s->actor_v);
  OSA_REQUIRE(s->adam_step && s->mult && s->step);
  OSA_REQUIRE(data->obs && data->act && data->reward && data->cost && data->next_obs && data->done && data->init_obs);
  OSA_REQUIRE(data->n_rows >= 1 && data->ld_obs >= lo.D && data->ld_next >= lo.D && data->ld_init >= lo.D &&
              data->ld_act >= lo.A);
  OSA_REQUIRE(dr->idx && dr->nslots >= 1);
  OSA_REQUIRE(hp->alpha > 0.f && hp->beta1 >= 0.0 && hp->beta1 < 1.0 && hp->beta2 >= 0.0 && hp->beta2 < 1.0);
  for (const float* p : {s->nu, s->nu_m, s->nu_v, s->chi, s->chi_m, s->chi_v, s->actor, s->actor_m, s->actor_v})
    OSA_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0);
  const DCtx c = {dr->idx, s->step, dr->nslots, lo.B, data->n_rows, hp->route == OSA_DICE_ROUTE_SINGLE, osa_stream(stream)};
  hipStream_t st = c.st;
  const int B = lo.B;
  float *h[3][GM_MAXL], *z[3][2], *grad[3];
  for (int k = 0; k < 3; ++k) {
    for (int l = 0; l < GM_MAXL; ++l) h[k][l] = ws + w.h[k][l];
    for (int q = 0; q < 2; ++q) z[k][q] = ws + w.z[k][q];
    grad[k] = ws + w.grad[k];
  }
  float* dout[2] = {ws + w.dout[0], ws + w.dout[1]};
  const float* params[3] = {s->nu, s->chi, s->actor};
  const DSrc x = dice_gather(data, B);
  for (int it = 0; it < nsteps; ++it) {
    int rc;
    // 1. nu and chi over obs[idx] || next_obs[idx] || init_obs[idx]
    DNetJob fw[2];
    for (int k = 0; k < 2; ++k) fw[k] = {&lo.n[k], params[k], x, 3 * B, h[k], nullptr, grad[k], lo.n[k].L - 1};
    if ((rc = dice_forward(c, fw, 2)) != OSA_OK) return rc;
    // 2. heads, losses, multipliers
    DHead hd = {};
    for (int k = 0; k < 2; ++k) {
      const CNet& n = lo.n[k];
      const int t = n.L - 1;
      hd.h[k] = h[k][t - 1]; hd.ldh[k] = n.ldh[t - 1]; hd.K[k] = n.in[t]; hd.ldw[k] = n.ld[t];
      hd.w[k] = params[k] + n.oW[t]; hd.b[k] = params[k] + n.ob[t];
      hd.dout[k] = dout[k]; hd.gw[k] = grad[k] + n.oW[t]; hd.gb[k] = grad[k] + n.ob[t];
    }
    hd.reward = data->reward; hd.cost = data->cost; hd.done = data->done; hd.idx = dr->idx; hd.step = s->step;
    hd.nrows = data->n_rows; hd.nslots = dr->nslots; hd.B = B; hd.fn = lo.fn;
    hd.gamma = hp->gamma; hd.alpha = hp->alpha; hd.cost_limit = hp->cost_limit; hd.cost_ub_eps = hp->cost_ub_eps;
    hd.lr_lamb = hp->lr_lamb; hd.lr_tau = hp->lr_tau; hd.beta1 = hp->beta1; hd.beta2 = hp->beta2; hd.eps = hp->adam_eps;
    hd.mult = s->mult; hd.adam_step = s->adam_step; hd.stats = stats;
    hipLaunchKernelGGL(dice_heads_kernel, dim3(1), dim3(DH_THREADS), 0, st, hd);
    // 3. backward of both networks: the heads' dZ (a K = 1 product of the dL/d(output) column with the head's weights)
    // in one launch, then the networks below their heads, whose weight gradients the list kernel owns
    DProb ph[2];
    CNet body[2];
    DNetJob bw[2];
    for (int k = 0; k < 2; ++k) {
      const CNet& n = lo.n[k];
      const int l = n.L - 1;
      DProb& q = ph[k] = dl_prob();
      q.bt = 1;
      q.A = dl_plain(dout[k], 1);
      q.Bm = dl_plain(params[k] + n.oW[l], n.ld[l]);
      q.C = z[k][0]; q.ldc = n.ldh[l - 1];
      q.M = 3 * B; q.N = n.in[l]; q.K = 1;
      q.dact = n.act; q.aux = h[k][l - 1]; q.ldaux = n.ldh[l - 1];
      body[k] = n;
      body[k].L = l;
      bw[k] = {&body[k], params[k], x, 3 * B, h[k], z[k], grad[k], l};
    }
    if ((rc = dl_launch(c, ph, 2)) != OSA_OK) return rc;
    if ((rc = dice_backward(c, bw, 2)) != OSA_OK) return rc;
    DAdam ad = {};
    for (int k = 0; k < 2; ++k) {
      ad.params[k] = k == 0 ? s->nu : s->chi; ad.m[k] = k == 0 ? s->nu_m : s->chi_m; ad.v[k] = k == 0 ? s->nu_v : s->chi_v;
      ad.grad[k] = grad[k]; ad.Pn[k] = lo.n[k].Pn; ad.lr[k] = k == 0 ? hp->lr_nu : hp->lr_chi;
      ad.adam_step[k] = s->adam_step;
    }
    ad.beta1 = hp->beta1; ad.beta2 = hp->beta2; ad.eps = hp->adam_eps;
    const int pmax = ad.Pn[0] > ad.Pn[1] ? ad.Pn[0] : ad.Pn[1];
    hipLaunchKernelGGL(dice_adam_kernel, dim3(crr_blocks(pmax, 256), 2), dim3(256), 0, st, ad);
    // 4. the updated nu over obs || next_obs together with the actor over obs
    DNetJob f4[2];
    f4[0] = {&lo.n[0], s->nu, x, 2 * B, h[0], nullptr, nullptr, lo.n[0].L - 1};
    f4[1] = {&lo.n[2], s->actor, x, B, h[2], nullptr, nullptr, lo.n[2].L};
    if ((rc = dice_forward(c, f4, 2)) != OSA_OK) return rc;
    const CNet &nn = lo.n[0], &na = lo.n[2];
    DPolicy po = {};
    po.h = h[0][nn.L - 2]; po.ldh = nn.ldh[nn.L - 2]; po.K = nn.in[nn.L - 1];
    po.wv = s->nu + nn.oW[nn.L - 1]; po.bv = s->nu + nn.ob[nn.L - 1];
    po.reward = data->reward; po.cost = data->cost; po.done = data->done; po.act = data->act; po.ld_act = data->ld_act;
    po.idx = dr->idx; po.step = s->step; po.nrows = data->n_rows; po.nslots = dr->nslots; po.B = B; po.A = lo.A;
    po.lda = lo.lda; po.fn = lo.fn; po.gamma = hp->gamma; po.alpha = hp->alpha; po.mult = s->mult;
    po.mu = h[2][na.L - 1]; po.log_std = s->actor + na.oLS; po.w = ws + w.w; po.dz = z[2][0];
    po.g_log_std = grad[2] + na.oLS; po.stats = stats; po.adam_step = s->adam_step + 1;
    hipLaunchKernelGGL(dice_policy_kernel, dim3(1), dim3(DH_THREADS), 0, st, po);
    DNetJob ba = {&na, s->actor, x, B, h[2], z[2], grad[2], na.L};
    if ((rc = dice_backward(c, &ba, 1)) != OSA_OK) return rc;
    DAdam aa = {};
    aa.params[0] = s->actor; aa.m[0] = s->actor_m; aa.v[0] = s->actor_v; aa.grad[0] = grad[2]; aa.Pn[0] = na.Pn;
    aa.lr[0] = hp->lr_actor; aa.adam_step[0] = s->adam_step + 1;
    aa.beta1 = hp->beta1; aa.beta2 = hp->beta2; aa.eps = hp->adam_eps;
    hipLaunchKernelGGL(dice_adam_kernel, dim3(crr_blocks(na.Pn, 256), 1), dim3(256), 0, st, aa);
    hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(64), 0, st, s->actor + na.oLS, lo.A, stats, s->step, dr->nslots);
    OSA_CHECK_LAUNCH();
  }
  return OSA_OK;
}

int osa_dice_values(const osa_dice_desc* desc, int route, const float* nu, const float* chi, const float* obs, int ld_obs,
                    long n, float* out_nu, float* out_chi, float* ws, size_t ws_floats, void* stream) {
  DLayout lo;
  OSA_REQUIRE(desc && nu && chi && obs && out_nu && out_chi && ws && n >= 1);
  const int rc0 = dice_make_layout(desc, &lo);
  if (rc0 != OSA_OK) return rc0;
  OSA_REQUIRE(route == OSA_DICE_ROUTE_LIST || route == OSA_DICE_ROUTE_SINGLE);
  OSA_REQUIRE(n <= 3l * lo.B && ld_obs >= lo.D);  // (the step's workspace holds 3 B rows)
  const DWs w = dice_ws(lo);
  OSA_REQUIRE(ws_floats >= w.total && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  const DCtx c = {nullptr, nullptr, 1, 0, 0, route == OSA_DICE_ROUTE_SINGLE, osa_stream(stream)};
  float* h[2][GM_MAXL];
  const float* params[2] = {nu, chi};
  float* out[2] = {out_nu, out_chi};
  DNetJob fw[2];
  for (int k = 0; k < 2; ++k) {
    for (int l = 0; l < GM_MAXL; ++l) h[k][l] = ws + w.h[k][l];
    DSrc x = dl_plain(obs, ld_obs);
    x.vec = 0;  // (the caller's rows: any alignment)
    fw[k] = {&lo.n[k], params[k], x, (int)n, h[k], nullptr, nullptr, lo.n[k].L - 1};
  }
  const int rc = dice_forward(c, fw, 2);
  if (rc != OSA_OK) return rc;
  for (int k = 0; k < 2; ++k) {
    const CNet& nk = lo.n[k];
    const int t = nk.L - 1;
    hipLaunchKernelGGL(dice_dots_kernel, dim3(1), dim3(DH_THREADS), 0, c.st, h[k][t - 1], nk.ldh[t - 1], nk.in[t],
                       params[k] + nk.oW[t], params[k] + nk.ob[t], (int)n, out[k]);
  }
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

}  // extern "C"
