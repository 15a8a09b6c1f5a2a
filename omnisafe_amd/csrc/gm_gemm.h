// The float32-MFMA tile GEMM of the layer-wise paths: up to three problems per launch, fused epilogues.  Moved here
// unchanged from general_mlp.hip so that crr_kernels.hip (the offline CRR / CCRR step) runs its layers on the same
// kernel; both translation units include it and get their own instantiations.
#pragma once
#include <stdlib.h>

#include "skinny_mlp.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// ------------------------------------------------------------------------------------------------
// the GEMM
// ------------------------------------------------------------------------------------------------
struct GProb {
  const float* A;
  const float* B;
  float* C;
  const float* bias;   // epilogue: + bias[n]
  const float* aux;    // epilogue: * act'(aux[m][n])
  float* cb;           // ones_n >= 0: column ones_n of the product goes to cb[m] (the bias gradient)
  int M, N, K, lda, ldb, ldc, ldaux;
  int act;             // epilogue: activation code, or -1
  int dact;            // epilogue: activation code whose derivative multiplies, or -1
  int accumulate;      // C += product
  int ones_n;          // >= 0: B(k, ones_n) = 1 for every k (only with BT)
  int cb_pad;          // cb[M .. cb_pad) = 0 (padding of the bias block)
  long slab_stride;    // split s writes C + s * slab_stride and cb + s * slab_stride
  int splits;          // this problem's splits of K (<= GArgs.splits, the launch's grid.z per problem)
};
struct GArgs {
  GProb p[3];
  int nprob, splits;
  // != 0: XCD-aware tile order (+ 1 % at 1024 x 1024 / 16 384 rows: 3 960 v 3 998 us per step, same box).  Workgroup i of a launch lands on XCC i mod 8 (each with its own L2): in dispatch order
  // (x fastest) the 8 column tiles of a 1024-wide layer go to 8 DIFFERENT L2s and every one of them streams the whole
  // row operand.  Remapped, XCC c owns the row blocks c, c + 8, ... with ALL their column tiles: a row block is fetched
  // into one L2 once, the (small) column operand into every L2.  Same tiles, same arithmetic.
  int xcd;
};

// C[m][n] = epi(sum_k A(m, k) B(k, n)).   AT: A(m, k) = A[k lda + m] (else A[m lda + k]);
//                                          BT: B(k, n) = B[k ldb + n] (else B[n ldb + k]).
// BK: K step per LDS stage.  16 when the launch has enough workgroups to hide memory latency behind each other; 64
// when it has few (the skinny GEMMs of a 64-row minibatch stream megabytes of weights through a few dozen workgroups:
// a step of 16 with one tile of lookahead paid a full L2 round trip per 0.2 us of MFMA work -- 40-70 us per layer at
// hidden 1024; four times the bytes in flight per barrier).
template <int TM, int TN, int BK, bool AT, bool BT>
__global__ __launch_bounds__(256) void gm_gemm_kernel(GArgs g) {
  constexpr int LD = BK + 4, MI = TM / 64, NJ = TN / 64, UA = TM * BK / 1024, UB = TN * BK / 1024;
  // An operand that is contiguous along its tile-row index (AT / BT: the activations of the weight-gradient GEMM, the
  // weights of the backward-data GEMM) stays K-MAJOR in LDS -- [k][row], leading dimension rows + 8 -- instead of being
  // transposed on the way in: 16-byte global loads with a wave on 1 KB of consecutive bytes and 16-byte LDS stores, where
  // the transposing stores were four scalar writes per piece from 64-byte row segments; the MFMA fragments then are four
  // scalar LDS reads of 32 consecutive floats per lane group (the two lane groups 4 rows = 32 banks apart) instead of
  // one 16-byte read.  Same values into the same MFMAs: same bits.
  constexpr int LDTA = TM + 8, LDTB = TN + 8;
  constexpr int SZA = AT ? BK * LDTA : TM * LD, SZB = BT ? BK * LDTB : TN * LD;
  extern __shared__ __attribute__((aligned(16))) float gm_smem[];
  float(*sA)[SZA] = reinterpret_cast<float(*)[SZA]>(gm_smem);
  float(*sB)[SZB] = reinterpret_cast<float(*)[SZB]>(gm_smem + 2 * SZA);
  const int pi = blockIdx.z / g.splits, sp = blockIdx.z - pi * g.splits;
  // (selected with scalar moves: a run-time index into the by-value argument would go through scratch memory)
  const GProb p = pi == 0 ? g.p[0] : (pi == 1 ? g.p[1] : g.p[2]);
  const int M = p.M, N = p.N, K = p.K;
  const int ncols = N + (p.ones_n >= 0 ? 1 : 0);
  int bx = blockIdx.x, by = blockIdx.y;
  if (g.xcd && (gridDim.y & 7) == 0) {
    const int gx = gridDim.x, lid = bx + gx * by, xcd = lid & 7, slot = lid >> 3;
    by = (slot / gx) * 8 + xcd;
    bx = slot - (slot / gx) * gx;
  }
  const int m0 = by * TM, n0 = bx * TN;
  if (m0 >= M || n0 >= (ncols > p.ldc ? ncols : p.ldc) || sp >= p.splits) return;
  int kper = (K + p.splits - 1) / p.splits;
  kper = (kper + BK - 1) / BK * BK;
  const int kbeg = sp * kper;
  const int kend = K < kbeg + kper ? K : kbeg + kper;
  const int nkt = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
  const int wm = (wave >> 1) * (TM / 2), wn = (wave & 1) * (TN / 2);
  const float* __restrict__ A = p.A;
  const float* __restrict__ B = p.B;
  f32x4 ra[UA], rb[UB];
  auto load_tile = [&](int kt) {
    const int k0 = kbeg + kt * BK;
#pragma unroll
    for (int q = 0; q < UA; ++q) {
      const int u = tid + 256 * q;
      if constexpr (!AT) {
        const int r = u / (BK / 4), c = u % (BK / 4), m = m0 + r;
        ra[q] = gm_load4(A + (long)m * p.lda, k0 + 4 * c, kend, m < M);
      } else {
        const int kq = u / (TM / 4), c = u % (TM / 4), k = k0 + kq;
        ra[q] = gm_load4(A + (long)k * p.lda, m0 + 4 * c, M, k < kend);
      }
    }
#pragma unroll
    for (int q = 0; q < UB; ++q) {
      const int u = tid + 256 * q;
      if constexpr (!BT) {
        const int r = u / (BK / 4), c = u % (BK / 4), n = n0 + r;
        rb[q] = gm_load4(B + (long)n * p.ldb, k0 + 4 * c, kend, n < N);
      } else {
        const int kq = u / (TN / 4), c = u % (TN / 4);
        const int k = k0 + kq, nn = n0 + 4 * c;
        f32x4 v = gm_load4(B + (long)k * p.ldb, nn, N, k < kend);
        if (p.ones_n >= 0 && k < kend) {  // the column of ones that turns the bias gradient into one more output column
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (nn + i == p.ones_n) v[i] = 1.f;
        }
        rb[q] = v;
      }
    }
  };
  auto store_tile = [&](int st) {
#pragma unroll
    for (int q = 0; q < UA; ++q) {
      const int u = tid + 256 * q;
      if constexpr (!AT) {
        *reinterpret_cast<f32x4*>(&sA[st][(u / (BK / 4)) * LD + 4 * (u % (BK / 4))]) = ra[q];
      } else {
        *reinterpret_cast<f32x4*>(&sA[st][(u / (TM / 4)) * LDTA + 4 * (u % (TM / 4))]) = ra[q];
      }
    }
#pragma unroll
    for (int q = 0; q < UB; ++q) {
      const int u = tid + 256 * q;
      if constexpr (!BT) {
        *reinterpret_cast<f32x4*>(&sB[st][(u / (BK / 4)) * LD + 4 * (u % (BK / 4))]) = rb[q];
      } else {
        *reinterpret_cast<f32x4*>(&sB[st][(u / (TN / 4)) * LDTB + 4 * (u % (TN / 4))]) = rb[q];
      }
    }
  };
  f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  if (nkt > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int st = kt & 1;
    if (kt + 1 < nkt) load_tile(kt + 1);  // the next tile's global loads are in flight under this tile's MFMAs
#pragma unroll
    for (int s = 0; s < BK / 8; ++s) {
      // K permutation inside a block of 8: lane group kk consumes k = 8 s + 4 kk + j in MFMA step j, for A and B
      // alike -- each fragment is ONE 16-byte LDS read per lane and feeds four MFMAs
      f32x4 af[MI], bf[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        if constexpr (!AT) {
          af[i] = *reinterpret_cast<const f32x4*>(&sA[st][(wm + 32 * i + l31) * LD + 8 * s + 4 * kk]);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) af[i][q] = sA[st][(8 * s + 4 * kk + q) * LDTA + wm + 32 * i + l31];
        }
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if constexpr (!BT) {
          bf[j] = *reinterpret_cast<const f32x4*>(&sB[st][(wn + 32 * j + l31) * LD + 8 * s + 4 * kk]);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) bf[j][q] = sB[st][(8 * s + 4 * kk + q) * LDTB + wn + 32 * j + l31];
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][q], bf[j][q], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) store_tile(st ^ 1);
    __syncthreads();
  }
  // ---- epilogue: D[row = (r & 3) + 8 (r >> 2) + 4 kk][col = l31] of every 32 x 32 tile
  float* __restrict__ C = p.C + (long)sp * p.slab_stride;
  float* __restrict__ cb = p.cb ? p.cb + (long)sp * p.slab_stride : nullptr;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = n0 + wn + 32 * j + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * kk;
        float v = acc[i][j][r];
        if (m < M) {
          if (n < N) {
            float* dst = C + (long)m * p.ldc + n;
            if (p.accumulate) v += *dst;
            if (p.bias) v += p.bias[n];
            if (p.act >= 0) v = gm_act(v, p.act);
            if (p.dact >= 0) v *= gm_dact(p.aux[(long)m * p.ldaux + n], p.dact);
            *dst = v;
          } else {
            if (n == p.ones_n && cb) cb[m] = v;
            if (n < p.ldc && p.ones_n >= 0) C[(long)m * p.ldc + n] = 0.f;  // padding columns of the weight block
          }
        } else if (n == p.ones_n && cb && m < p.cb_pad) {
          cb[m] = 0.f;  // padding of the bias block
        }
      }
    }
}

int gm_xcd_order() {  // (A/B switch, read once: OSA_GMLP_XCD_ORDER=0 keeps the dispatch order)
  static const int xcd_sw = [] {
    const char* v = getenv("OSA_GMLP_XCD_ORDER");
    return (v != nullptr && v[0] == '0' && v[1] == 0) ? 0 : 1;
  }();
  return xcd_sw;
}

template <int TM, int TN, int BK, bool AT, bool BT>
int gm_launch(const GArgs& g_, int maxM, int maxN, hipStream_t st) {
  GArgs g = g_;
  g.xcd = gm_xcd_order();
  constexpr size_t lds = (size_t)2 * ((AT ? BK * (TM + 8) : TM * (BK + 4)) + (BT ? BK * (TN + 8) : TN * (BK + 4))) * sizeof(float);
  if constexpr (lds > 64 * 1024) {
    static OsaPerDeviceOnce attr_set;
    if (attr_set.need()) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gm_gemm_kernel<TM, TN, BK, AT, BT>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return OSA_EHIP;
      attr_set.set();
    }
  }
  dim3 grid((maxN + TN - 1) / TN, (maxM + TM - 1) / TM, g.nprob * g.splits);
  hipLaunchKernelGGL((gm_gemm_kernel<TM, TN, BK, AT, BT>), grid, dim3(256), lds, st, g);
  return hipGetLastError() == hipSuccess ? OSA_OK : OSA_EHIP;
}

#ifndef GM_BK
#define GM_BK 16  // K step of the launches with enough workgroups (A/B: -DGM_BK=32)
#endif

// ---- the launch plan.  Which kernel a launch takes, how a K range is sliced and which launches a skinny step fuses are
// pure host functions of the shapes (gm_pick_tile, gm_rows_plan, gs_plan, gm_splits) that the launchers themselves
// call; osa_gmlp_plan walks the same launchers with a recorder set and `dry` on, so that what it reports is what a step
// of this process does -- the once-per-process switches (OSA_GMLP_DEEP, _XCD_ORDER, _ROW_SPLIT, _TOP_FUSE) included.
struct GPlanRec {
  int* out;
  int n, cap;
  bool dry;          // record only: nothing is launched, no pointer is followed
  int rowS, Si[3];   // the row split of the launch about to be recorded (gm_gemm_rows), 0: none
  int launches;
};
thread_local GPlanRec* gm_plan = nullptr;
inline void gm_plan_put(int v) {
  if (gm_plan->n < gm_plan->cap) gm_plan->out[gm_plan->n] = v;
  ++gm_plan->n;
}

// the tile of one grouped launch follows its largest problem (64-wide tiles for skinny ones), the K step the number
// of workgroups the launch will have
struct GTile {
  int TM, TN, BK;
};
GTile gm_pick_tile(int maxM, int maxN, int nprob, int splits) {
  bool bigM = maxM > 64, bigN = maxN > 64;
  auto count = [&](int tm, int tn) {
    return (long)((maxM + tm - 1) / tm) * ((maxN + tn - 1) / tn) * nprob * splits;
  };
  // a launch that would leave most of the chip idle takes the 64-wide tiles (twice / four times the workgroups)
  if (bigN && count(bigM ? 128 : 64, 128) < 128) bigN = false;
  if (bigM && count(128, bigN ? 128 : 64) < 128) bigM = false;
  const long wgs = count(bigM ? 128 : 64, bigN ? 128 : 64);
  static const int deep_sw = [] {  // (A/B switch: OSA_GMLP_DEEP=0 / 1 forces the K step 16 / 64)
    const char* v = getenv("OSA_GMLP_DEEP");
    return v == nullptr ? -1 : (v[0] == '1' ? 1 : 0);
  }();
  const bool deep = deep_sw >= 0 ? deep_sw == 1 : wgs < 256;  // few workgroups: latency-bound -> K step 64
  return GTile{bigM ? 128 : 64, bigN ? 128 : 64, deep ? 64 : GM_BK};
}

// one grouped launch
template <bool AT, bool BT>
int gm_gemm(const GArgs& g, hipStream_t st) {
  int maxM = 0, maxN = 0;
  for (int i = 0; i < g.nprob; ++i) {
    const int nc = g.p[i].ones_n >= 0 ? (g.p[i].ldc > g.p[i].N + 1 ? g.p[i].ldc : g.p[i].N + 1) : g.p[i].N;
    if (g.p[i].M > maxM) maxM = g.p[i].M;
    if (nc > maxN) maxN = nc;
  }
  if (g.nprob == 0 || maxM == 0) return OSA_OK;
  const GTile t = gm_pick_tile(maxM, maxN, g.nprob, g.splits);
  if (gm_plan) {  // one record per launch: OSA_GMLP_PLAN_LAUNCH ints
    gm_plan_put(t.TM); gm_plan_put(t.TN); gm_plan_put(t.BK); gm_plan_put(AT); gm_plan_put(BT); gm_plan_put(g.splits);
    gm_plan_put(gm_plan->rowS);
    gm_plan_put(g.nprob);
    for (int i = 0; i < 3; ++i) gm_plan_put(gm_plan->rowS && i < g.nprob ? gm_plan->Si[i] : 0);
    for (int i = 0; i < 3; ++i) gm_plan_put(i < g.nprob ? g.p[i].splits : 0);
    gm_plan_put(gm_xcd_order());
    gm_plan->rowS = 0;
    ++gm_plan->launches;
    if (gm_plan->dry) return OSA_OK;
  }
  const bool deep = t.BK == 64;
#define GM_GO(TM_, TN_)                                                              \
  return deep ? gm_launch<TM_, TN_, 64, AT, BT>(g, maxM, maxN, st) : gm_launch<TM_, TN_, GM_BK, AT, BT>(g, maxM, maxN, st)
  if (t.TM == 128 && t.TN == 128) GM_GO(128, 128);
  if (t.TM == 128) GM_GO(128, 64);
  if (t.TN == 128) GM_GO(64, 128);
  GM_GO(64, 64);
#undef GM_GO
}

}  // namespace
