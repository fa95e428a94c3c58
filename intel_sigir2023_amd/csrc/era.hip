// ERA baseline (Evolutionary Rank Aggregation; models/supervise/ERA.py + ERARunner.py of the reference): a genetic algorithm over
// the weights of a tiny MLP that scores every item from rank features of the base rankers.  The reference evaluates one solution at
// a time (pygad.torchga.predict + the numpy evaluate_method, ERARunner.py:138-148); here one launch scores the whole population:
//   era_features_kernel   the per-item features of ERA.Dataset._get_feed_dict (ERA.py:54-65), one wave per session;
//   era_fitness_kernel    MLP of every solution over every item + the "All" NDCG@1 of evaluate_method (ERARunner.py:87-97): a wave owns a
//                         session, its lanes keep their items' features and labels in registers for all P solutions; a solution's weights
//                         are wave-uniform and read through uniform (scalar-cache) loads, so the inner products are VALU FMAs with a scalar
//                         operand.  Per-workgroup partial sums go to a workspace, era_gain_reduce_kernel adds them in a fixed order.
#include "era.h"

#define ERA_PC 256       // solutions per workgroup (grid.y chunks); = the block size

namespace {

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// lane exchange inside a row of 16 lanes on the VALU (DPP), no LDS round trip: quad_perm [1,0,3,2] and [2,3,0,1] are the xor-1 / xor-2
// butterflies; row_half_mirror (lane i <-> 7 - i of its 8) and row_mirror (i <-> 15 - i) pair each quad / each half with the other one,
// which is all a reduction needs once the lanes of a quad (of a half) already agree
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) { return __int_as_float(dpp_i<CTRL>(__float_as_int(v))); }
#define ERA_DPP_XOR1 0xB1
#define ERA_DPP_XOR2 0x4E
#define ERA_DPP_HALF_MIRROR 0x141
#define ERA_DPP_MIRROR 0x140

// (bv, bl) <- the better of it and (ov, ol): larger prediction, among equal predictions the smaller label
__device__ __forceinline__ void era_take(float& bv, int& bl, float ov, int ol) {
  const bool take = (ov > bv) | ((ov == bv) & (ol < bl));
  bv = take ? ov : bv;
  bl = take ? ol : bl;
}

// ---- rank features ----------------------------------------------------------------------------------------------------------------
// rank_m(l) = 1 + #{j < len : s_m(j) > s_m(l) or (s_m(j) == s_m(l) and j > l)}: np.argsort(x)[::-1] in its stable form (ERA.py:58-59)
__global__ __launch_bounds__(256) void era_features_kernel(const float* __restrict__ scores, const int* __restrict__ slen, int B, int L, int K,
                                                           int window, float* __restrict__ feat) {
  __shared__ float sc[4][(ERA_MAX_F - 2) * ERA_MAX_L];       // [m][l] per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  const bool live = b < B;
  const int len = live ? min(max(slen[b], 0), L) : 0;
  const int F = K + 2;
  for (int l = lane; l < len; l += 64)
    for (int m = 0; m < K; ++m) sc[wave][m * ERA_MAX_L + l] = scores[((size_t)b * L + l) * K + m];
  __syncthreads();
  if (!live) return;
  for (int l = lane; l < L; l += 64) {
    float* out = feat + ((size_t)b * L + l) * F;
    if (l >= len) {
      for (int f = 0; f < F; ++f) out[f] = 0.f;
      continue;
    }
    int p10 = 0, r0 = 0, r1 = 0;
    for (int m = 0; m < K; ++m) {
      const float* s = &sc[wave][m * ERA_MAX_L];
      const float sl = s[l];
      int rank = 1;
      for (int j = 0; j < len; ++j) {
        const float sj = s[j];
        rank += (sj > sl || (sj == sl && j > l)) ? 1 : 0;
      }
      p10 += rank <= 10;
      if (m == 0) r0 = rank;
      if (m == 1) r1 = rank;
      out[2 + m] = (float)(1.0 - (double)(rank - 1) / (double)len);       // ERA.py:60 in float64, then .float() (:43)
    }
    out[0] = (float)p10;                                                  // ERA.py:64
    out[1] = abs(r1 - r0) <= window ? 0.5f : 0.f;                         // ERA.py:65
  }
}

// ---- population fitness -----------------------------------------------------------------------------------------------------------
// pop [P, G]: per Linear weight [out, in] row-major then bias [out] (pygad.torchga: the state_dict order of ERA.mlp, ERA.py:31-37).
// grid (workgroups of 4 * spw sessions, chunks of ERA_PC solutions); part [P, gridDim.x] per-workgroup sums of the gains.
// NH == 2: the first hidden layer of the lane's current item goes through LDS (hs [4 waves][H1][64 lanes], dynamic).
// HT > 0 (NH == 1): the hidden width as a compile-time constant -- every weight of a solution sits at an immediate offset from one base
// and the unit loop unrolls, which takes the address arithmetic of the run-time-width loop off the scalar unit.
template <int F, int IPL, int NH, int HT>
__global__ __launch_bounds__(256) void era_fitness_kernel(const float* __restrict__ pop, const float* __restrict__ feat,
                                                          const int* __restrict__ ranking, const int* __restrict__ slen, int P, int B, int L,
                                                          int H1rt, int H2, int G, int width, int spw, double* __restrict__ part,
                                                          float* __restrict__ pred_out) {
  const int H1 = HT > 0 ? HT : H1rt;
  extern __shared__ float hs[];
  __shared__ double wacc[4][ERA_PC];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p0 = blockIdx.y * ERA_PC;
  const int np = min(ERA_PC, P - p0);
  for (int t = threadIdx.x; t < 4 * ERA_PC; t += 256) (&wacc[0][0])[t] = 0.0;
  __syncthreads();

  for (int s = 0; s < spw; ++s) {
    const int b = (blockIdx.x * 4 + wave) * spw + s;
    if (b >= B) break;
    const int len = min(max(slen[b], 0), L);
    float x[IPL][F];
    int lab[IPL];
    bool valid[IPL];
    int maxlab = 0;
#pragma unroll
    for (int i = 0; i < IPL; ++i) {
      const int l = lane + 64 * i;
      valid[i] = l < len;
      const size_t row = (size_t)b * L + (valid[i] ? l : 0);
#pragma unroll
      for (int f = 0; f < F; ++f) x[i][f] = valid[i] ? feat[row * F + f] : 0.f;
      lab[i] = valid[i] ? max(ranking[row], 0) : 0;                     // ERARunner.py:57
      maxlab = max(maxlab, lab[i]);
    }
    maxlab = wave_max_i(maxlab);
    const double denom = (double)max(1, maxlab);                        // idcg == 0 -> 1 (ERARunner.py:95)
    const bool has_pad = len < width;                                   // one pad candidate: prediction 0, label 0 (ERARunner.py:45-57)

    for (int pc = 0; pc < np; pc += 64) {
      const int nq = min(64, np - pc);
      int wl = 0x7fffffff;
      for (int q = 0; q < nq; ++q) {
        const int p = p0 + pc + q;
        const float* __restrict__ w = pop + (size_t)p * G;
        const float* W1 = w;
        const float* b1 = w + H1 * F;
        float out[IPL];
        if (NH == 1) {
          const float* W2 = b1 + H1;
          const float b2 = W2[H1];
#pragma unroll
          for (int i = 0; i < IPL; ++i) out[i] = b2;
#pragma unroll(HT > 0 ? HT : 4)
          for (int j = 0; j < H1; ++j) {
            const float bj = b1[j], wj = W2[j];
#pragma unroll
            for (int i = 0; i < IPL; ++i) {
              float a = bj;
#pragma unroll
              for (int f = 0; f < F; ++f) a = fmaf(W1[j * F + f], x[i][f], a);
              out[i] = fmaf(wj, fmaxf(a, 0.f), out[i]);
            }
          }
        } else {
          const float* W2 = b1 + H1;
          const float* b2 = W2 + H2 * H1;
          const float* W3 = b2 + H2;
          const float b3 = W3[H2];
          float* my = hs + (size_t)wave * H1 * 64 + lane;
#pragma unroll
          for (int i = 0; i < IPL; ++i) {
            for (int j = 0; j < H1; ++j) {
              float a = b1[j];
#pragma unroll
              for (int f = 0; f < F; ++f) a = fmaf(W1[j * F + f], x[i][f], a);
              my[j * 64] = fmaxf(a, 0.f);
            }
            float o = b3;
            for (int k0 = 0; k0 < H2; k0 += 4) {
              int kk[4];
              float acc[4];
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                kk[c] = min(k0 + c, H2 - 1);
                acc[c] = b2[kk[c]];
              }
              for (int j = 0; j < H1; ++j) {
                const float hv = my[j * 64];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = fmaf(W2[kk[c] * H1 + j], hv, acc[c]);
              }
#pragma unroll
              for (int c = 0; c < 4; ++c)
                if (k0 + c < H2) o = fmaf(W3[k0 + c], fmaxf(acc[c], 0.f), o);
            }
            out[i] = o;
          }
        }
        if (pred_out) {
#pragma unroll
          for (int i = 0; i < IPL; ++i) {
            const int l = lane + 64 * i;
            if (l < L) pred_out[((size_t)p * B + b) * L + l] = valid[i] ? out[i] : 0.f;
          }
        }
        // winner: largest prediction, among equal predictions the smallest label (the rule of ndcg_kernel, optim.hip)
        float bv = -INFINITY;
        int bl = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < IPL; ++i) {       // selects, not branches: every lane runs the same instructions
          const bool take = valid[i] & ((out[i] > bv) | ((out[i] == bv) & (lab[i] < bl)));
          bv = take ? out[i] : bv;
          bl = take ? lab[i] : bl;
        }
        era_take(bv, bl, dpp_f<ERA_DPP_XOR1>(bv), dpp_i<ERA_DPP_XOR1>(bl));
        era_take(bv, bl, dpp_f<ERA_DPP_XOR2>(bv), dpp_i<ERA_DPP_XOR2>(bl));
        era_take(bv, bl, dpp_f<ERA_DPP_HALF_MIRROR>(bv), dpp_i<ERA_DPP_HALF_MIRROR>(bl));
        era_take(bv, bl, dpp_f<ERA_DPP_MIRROR>(bv), dpp_i<ERA_DPP_MIRROR>(bl));
        era_take(bv, bl, __shfl_xor(bv, 16), __shfl_xor(bl, 16));
        era_take(bv, bl, __shfl_xor(bv, 32), __shfl_xor(bl, 32));
        if (has_pad & ((0.f > bv) | ((0.f == bv) & (0 < bl)))) bl = 0;
        wl = lane == q ? bl : wl;       // lane q keeps the winner's label of solution pc + q
      }
      // one division per solution, by the lane that holds it; no candidate at all (empty session, width 0): gain 0
      wacc[wave][pc + lane] += (lane < nq && wl != 0x7fffffff) ? (double)wl / denom : 0.0;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < np) part[(size_t)(p0 + t) * gridDim.x + blockIdx.x] = ((wacc[0][t] + wacc[1][t]) + wacc[2][t]) + wacc[3][t];
}

// gain_sum[p] += sum over the workgroups' partials, in a fixed order (thread t takes g = t, t + 256, ..; then a fixed LDS tree)
__global__ __launch_bounds__(256) void era_gain_reduce_kernel(const double* __restrict__ part, int nwg, double* __restrict__ gain_sum) {
  __shared__ double sh[256];
  const int p = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (int g = t; g < nwg; g += 256) s += part[(size_t)p * nwg + g];
  sh[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) gain_sum[p] += sh[0];
}

// sessions per wave: a function of B alone, so that a launch's summation order depends on nothing but its shape.  Small enough that a
// large batch is several rounds of resident waves (7 per SIMD: 7168 on the chip) and the last, partly filled round stays a small share
inline int era_spw(int B) { return min(8, max(1, B / 32768)); }
inline int era_nwg(int B) { return cdiv(B, 4 * era_spw(B)); }

template <int F, int IPL>
int era_fitness_launch(int NH, dim3 grid, size_t lds, hipStream_t st, double work, const float* pop, const float* feat, const int* ranking,
                       const int* slen, int P, int B, int L, int H1, int H2, int G, int width, int spw, double* part, float* pred_out) {
  if (NH == 1 && H1 == 16) {       // the reference's default --hidden_sizes
    LAUNCH_W(work, 0.0, (era_fitness_kernel<F, IPL, 1, 16>), grid, dim3(256), 0, st, pop, feat, ranking, slen, P, B, L, H1, H2, G, width, spw, part, pred_out);
  } else if (NH == 1) {
    LAUNCH_W(work, 0.0, (era_fitness_kernel<F, IPL, 1, 0>), grid, dim3(256), 0, st, pop, feat, ranking, slen, P, B, L, H1, H2, G, width, spw, part, pred_out);
  } else {
    allow_lds(era_fitness_kernel<F, IPL, 2, 0>, lds);
    LAUNCH_W(work, 0.0, (era_fitness_kernel<F, IPL, 2, 0>), grid, dim3(256), lds, st, pop, feat, ranking, slen, P, B, L, H1, H2, G, width, spw, part, pred_out);
  }
  INTEL_CHECK_LAUNCH();
  return 0;
}

}  // namespace

int launch_era_features(int B, int L, int K, const float* scores, const int* slen, int window, float* feat, hipStream_t st) {
  INTEL_CHECK_ARG(K >= 2 && K + 2 <= ERA_MAX_F, "era_features: K=%d base rankers unsupported (2 <= K <= %d)", K, ERA_MAX_F - 2);
  INTEL_CHECK_ARG(L >= 1 && L <= ERA_MAX_L, "era_features: list length %d unsupported (1 <= L <= %d)", L, ERA_MAX_L);
  INTEL_CHECK_ARG(window >= 0, "era_features: window %d < 0", window);
  if (B <= 0) return 0;
  LAUNCH(era_features_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, scores, slen, B, L, K, window, feat);
  INTEL_CHECK_LAUNCH();
  return 0;
}

int era_genes(int F, int n_hidden, const int* hidden) {
  int G = 0, in = F;
  for (int i = 0; i < n_hidden; ++i) {
    G += hidden[i] * in + hidden[i];
    in = hidden[i];
  }
  return G + in + 1;
}

size_t era_fitness_ws_bytes(int P, int B) {
  if (P <= 0 || B <= 0) return 0;
  return rup_sz((size_t)era_nwg(B) * P * sizeof(double), 256);
}

int launch_era_fitness(int P, int B, int L, int F, int n_hidden, const int* hidden, const float* pop, const float* feat, const int* ranking,
                       const int* slen, int width, double* gain_sum, float* pred_out, void* ws, hipStream_t st) {
  INTEL_CHECK_ARG(P >= 1, "era_fitness: population of %d solutions", P);
  INTEL_CHECK_ARG(L >= 1 && L <= ERA_MAX_L, "era_fitness: list length %d unsupported (1 <= L <= %d)", L, ERA_MAX_L);
  INTEL_CHECK_ARG(F >= 4 && F <= ERA_MAX_F, "era_fitness: %d features unsupported (4 <= F <= %d)", F, ERA_MAX_F);
  INTEL_CHECK_ARG(hidden && n_hidden >= 1 && n_hidden <= ERA_MAX_HIDDEN, "era_fitness: %d hidden layers unsupported (1 <= n_hidden <= %d)", n_hidden,
                  ERA_MAX_HIDDEN);
  for (int i = 0; i < n_hidden; ++i)
    INTEL_CHECK_ARG(hidden[i] >= 1 && hidden[i] <= ERA_MAX_H, "era_fitness: hidden width %d unsupported (1 <= width <= %d)", hidden[i], ERA_MAX_H);
  INTEL_CHECK_ARG((long long)P * B * L < (1ll << 40), "era_fitness: P * B * L too large");
  if (B <= 0) return 0;
  const int H1 = hidden[0], H2 = n_hidden > 1 ? hidden[1] : 0;
  const int G = era_genes(F, n_hidden, hidden);
  const int spw = era_spw(B), nwg = era_nwg(B);
  const dim3 grid(nwg, cdiv(P, ERA_PC));
  const size_t lds = n_hidden > 1 ? (size_t)4 * H1 * 64 * sizeof(float) : 0;
  double* part = (double*)ws;
  const double work = 2.0 * (double)P * B * L * (G - 1);
  int rc = -1;
#define ERA_CASE(F_, IPL_)                                                                                                                  \
  rc = era_fitness_launch<F_, IPL_>(n_hidden, grid, lds, st, work, pop, feat, ranking, slen, P, B, L, H1, H2, G, width, spw, part, pred_out)
#define ERA_IPL(F_)                    \
  do {                                 \
    if (L <= 64) ERA_CASE(F_, 1);      \
    else if (L <= 128) ERA_CASE(F_, 2); \
    else ERA_CASE(F_, 4);              \
  } while (0)
  switch (F) {
    case 4: ERA_IPL(4); break;
    case 5: ERA_IPL(5); break;
    case 6: ERA_IPL(6); break;
    case 7: ERA_IPL(7); break;
    default: ERA_IPL(8); break;
  }
#undef ERA_IPL
#undef ERA_CASE
  if (rc) return rc;
  LAUNCH(era_gain_reduce_kernel, dim3(P), dim3(256), 0, st, part, nwg, gain_sum);
  INTEL_CHECK_LAUNCH();
  return 0;
}
