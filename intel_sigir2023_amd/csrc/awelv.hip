// aWELv baseline (models/supervise/aWELv.py of the reference; Liu, Du, Wu, JMLR 23 (2022)): a user embedding table E [users, H] and a
// base-ranker embedding table M [K, H]; a session of user u fuses its K base scores with w = softmax_k(E[u] . M[k]) (aWELv.py:26-40).
//   awelv_fwd_kernel          a wave owns a session (4 per workgroup): lanes over h (one float4 each) for the K inner products, then lanes
//                             over l for ens and the broadcast weights.  E[u] and M are read once per session, no LDS.
//   awelv_bwd_kernel          the same ownership over a grid-stride loop (at most AWELV_BWD_MAX_WG workgroups): K sums over l per lane,
//                             wave_sum, the softmax backward in its pairwise form, float atomics into the user's gradient row (a user may
//                             occur several times in a batch: the choice of scatter_add_rows_kernel), the M gradient kept in registers
//                             over the loop and left as one partial per workgroup.
//   awelv_dmodel_reduce_kernel  adds the partials in a fixed order: d_model_table is bit-reproducible without float atomics.
#include "awelv.h"

namespace {

// KT: compile-time bound of the k loops (4 or AWELV_KMAX), so that every per-k value stays in a register; K <= KT is wave-uniform
template <int KT>
__global__ __launch_bounds__(256) void awelv_fwd_kernel(const float* __restrict__ E, long long users, const float* __restrict__ M,
                                                        const int* __restrict__ u_id, const float* __restrict__ scores, int B, int L, int K,
                                                        int H, float* __restrict__ w, float* __restrict__ weights, float* __restrict__ ens) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  if (b >= B) return;
  const long long u = u_id[b];
  const bool ok = u >= 0 && u < users;       // an id outside the table: a zero embedding, never an access outside it
  const int h = lane * 4;
  const bool inh = h < H;
  f32x4 e = {0.f, 0.f, 0.f, 0.f};
  if (ok && inh) e = *reinterpret_cast<const f32x4*>(E + (size_t)u * H + h);
  float z[KT];
  float zmax = -INFINITY;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    z[k] = 0.f;
    if (k < K) {
      f32x4 m = {0.f, 0.f, 0.f, 0.f};
      if (inh) m = *reinterpret_cast<const f32x4*>(M + (size_t)k * H + h);
      z[k] = wave_sum((e[0] * m[0] + e[1] * m[1]) + (e[2] * m[2] + e[3] * m[3]));
      zmax = fmaxf(zmax, z[k]);
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    z[k] = k < K ? expf(z[k] - zmax) : 0.f;
    sum += z[k];
  }
  const float inv = 1.f / sum;
  float mine = 0.f;       // lane k keeps w_k
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    z[k] *= inv;
    mine = lane == k ? z[k] : mine;
  }
  if (lane < K) w[(size_t)b * K + lane] = mine;
  // ens over the WHOLE padded list (the reference repeats w over dim 1 and does not mask)
  const float* sc = scores + (size_t)b * L * K;
  for (int l = lane; l < L; l += 64) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) a = fmaf(z[k], sc[(size_t)l * K + k], a);
    ens[(size_t)b * L + l] = a;
  }
  // weights[b, l, :] = w: flat over l * K + k, so that the stores of a wave are contiguous
  float* wt = weights + (size_t)b * L * K;
  const int LK = L * K;
  for (int i0 = 0; i0 < LK; i0 += 64) {
    const int i = i0 + lane;
    const float v = __shfl(mine, i % K);
    if (i < LK) wt[i] = v;
  }
}

// part [gridDim.x, K * H]: the workgroup's sum of dz[b, k] * E[u_b, :] over its sessions
template <int KT>
__global__ __launch_bounds__(256) void awelv_bwd_kernel(const float* __restrict__ E, long long users, const float* __restrict__ M,
                                                        const int* __restrict__ u_id, const float* __restrict__ scores,
                                                        const float* __restrict__ w, const float* __restrict__ d_ens,
                                                        const float* __restrict__ d_weights, int B, int L, int K, int H,
                                                        float* __restrict__ d_uid, unsigned char* __restrict__ row_flags,
                                                        float* __restrict__ part) {
  extern __shared__ float sh[];       // [4 waves][K * H]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane * 4;
  const bool inh = h < H;
  f32x4 acc[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int g = blockIdx.x; g * 4 < B; g += gridDim.x) {
    const int b = g * 4 + wave;
    if (b >= B) continue;
    const long long u = u_id[b];
    const bool ok = u >= 0 && u < users;
    // gw[k] = sum over ALL l < L of d_ens * scores + d_weights
    float gw[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) gw[k] = 0.f;
    const float* sc = scores + (size_t)b * L * K;
    const float* dw = d_weights ? d_weights + (size_t)b * L * K : nullptr;
    for (int l = lane; l < L; l += 64) {
      const float de = d_ens[(size_t)b * L + l];
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (k < K) {
          gw[k] = fmaf(de, sc[(size_t)l * K + k], gw[k]);
          if (dw) gw[k] += dw[(size_t)l * K + k];
        }
    }
    float wv[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      wv[k] = 0.f;
      if (k < K) {
        gw[k] = wave_sum(gw[k]);
        wv[k] = w[(size_t)b * K + k];
      }
    }
    // dz_k = w_k * sum_j w_j (gw_k - gw_j): w_k (gw_k - sum_j w_j gw_j) without the cancellation of a saturated softmax
    float dz[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < KT; ++j)
        if (j < K) s = fmaf(wv[j], gw[k] - gw[j], s);
      dz[k] = k < K ? wv[k] * s : 0.f;
    }
    if (!ok) continue;       // a zero embedding: no gradient row, no share of M's gradient
    if (inh) {
      const f32x4 e = *reinterpret_cast<const f32x4*>(E + (size_t)u * H + h);
      f32x4 du = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (k < K) {
          const f32x4 m = *reinterpret_cast<const f32x4*>(M + (size_t)k * H + h);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            du[c] = fmaf(dz[k], m[c], du[c]);
            acc[k][c] = fmaf(dz[k], e[c], acc[k][c]);
          }
        }
      float* dst = d_uid + (size_t)u * H + h;
#pragma unroll
      for (int c = 0; c < 4; ++c) atomicAdd(dst + c, du[c]);
    }
    if (row_flags && lane == 0) row_flags[u] = 1;
  }

  const int KH = K * H;
  if (inh) {
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) *reinterpret_cast<f32x4*>(sh + (size_t)wave * KH + k * H + h) = acc[k];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < KH; i += 256)
    part[(size_t)blockIdx.x * KH + i] = ((sh[i] + sh[KH + i]) + sh[2 * KH + i]) + sh[3 * KH + i];
}

// d_model_table[i] = sum over the workgroups' partials in index order
__global__ __launch_bounds__(256) void awelv_dmodel_reduce_kernel(const float* __restrict__ part, int nwg, int KH, float* __restrict__ d_model) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= KH) return;
  float s = 0.f;
  for (int g = 0; g < nwg; ++g) s += part[(size_t)g * KH + i];
  d_model[i] = s;
}

inline int awelv_bwd_nwg(int B) { return min(cdiv(B, 4), AWELV_BWD_MAX_WG); }

int awelv_check(const char* what, int B, int L, int K, int H, long long users) {
  INTEL_CHECK_ARG(B >= 1, "%s: batch of %d sessions", what, B);
  INTEL_CHECK_ARG(L >= 1, "%s: list length %d < 1", what, L);
  INTEL_CHECK_ARG(K >= 1 && K <= AWELV_KMAX, "%s: K=%d base rankers unsupported (1 <= K <= %d)", what, K, AWELV_KMAX);
  INTEL_CHECK_ARG(H >= 4 && H <= AWELV_HMAX && H % 4 == 0, "%s: hidden size %d unsupported (a multiple of 4, 4 <= H <= %d)", what, H, AWELV_HMAX);
  INTEL_CHECK_ARG(users >= 0, "%s: %lld users", what, users);
  INTEL_CHECK_ARG((long long)L * K < (1ll << 31), "%s: L * K too large", what);
  return 0;
}

}  // namespace

int launch_awelv_fwd(int B, int L, int K, int H, const float* uid_table, long long users, const float* model_table, const int* u_id,
                     const float* scores, float* w, float* weights, float* ens, hipStream_t st) {
  if (int rc = awelv_check("awelv_forward", B, L, K, H, users)) return rc;
  INTEL_CHECK_ARG((((uintptr_t)uid_table | (uintptr_t)model_table) & 15) == 0, "awelv_forward: tables must be 16-byte aligned");
  const double bytes = 4.0 * ((double)B * L * (2.0 * K + 1.0) + (double)B * (H + K + 1) + (double)K * H);
  const double flops = 2.0 * B * ((double)K * H + (double)L * K);
  if (K <= 4) {
    LAUNCH_W(flops, bytes, (awelv_fwd_kernel<4>), dim3(cdiv(B, 4)), dim3(256), 0, st, uid_table, users, model_table, u_id, scores, B, L, K, H, w, weights, ens);
  } else {
    LAUNCH_W(flops, bytes, (awelv_fwd_kernel<AWELV_KMAX>), dim3(cdiv(B, 4)), dim3(256), 0, st, uid_table, users, model_table, u_id, scores, B, L, K, H, w, weights, ens);
  }
  INTEL_CHECK_LAUNCH();
  return 0;
}

size_t awelv_bwd_ws_bytes(int B, int K, int H) {
  if (B <= 0 || K <= 0 || H <= 0) return 0;
  return rup_sz((size_t)awelv_bwd_nwg(B) * K * H * sizeof(float), 256);
}

int launch_awelv_bwd(int B, int L, int K, int H, const float* uid_table, long long users, const float* model_table, const int* u_id,
                     const float* scores, const float* w, const float* d_ens, const float* d_weights, float* d_uid_table,
                     unsigned char* row_flags, float* d_model_table, void* ws, hipStream_t st) {
  if (int rc = awelv_check("awelv_backward", B, L, K, H, users)) return rc;
  INTEL_CHECK_ARG((((uintptr_t)uid_table | (uintptr_t)model_table) & 15) == 0, "awelv_backward: tables must be 16-byte aligned");
  const int nwg = awelv_bwd_nwg(B), KH = K * H;
  const size_t lds = (size_t)4 * KH * sizeof(float);
  float* part = (float*)ws;
  const double bytes = 4.0 * ((double)B * L * (K + 1.0 + (d_weights ? K : 0)) + (double)B * (3.0 * H + K + 1) + (double)K * H);
  const double flops = 2.0 * B * ((double)L * K + 2.0 * K * H + (double)K * K);
  if (K <= 4) {
    allow_lds(awelv_bwd_kernel<4>, lds);
    LAUNCH_W(flops, bytes, (awelv_bwd_kernel<4>), dim3(nwg), dim3(256), lds, st, uid_table, users, model_table, u_id, scores, w, d_ens, d_weights, B, L, K, H,
             d_uid_table, row_flags, part);
  } else {
    allow_lds(awelv_bwd_kernel<AWELV_KMAX>, lds);
    LAUNCH_W(flops, bytes, (awelv_bwd_kernel<AWELV_KMAX>), dim3(nwg), dim3(256), lds, st, uid_table, users, model_table, u_id, scores, w, d_ens, d_weights, B, L,
             K, H, d_uid_table, row_flags, part);
  }
  INTEL_CHECK_LAUNCH();
  LAUNCH(awelv_dmodel_reduce_kernel, dim3(cdiv(KH, 256)), dim3(256), 0, st, part, nwg, KH, d_model_table);
  INTEL_CHECK_LAUNCH();
  return 0;
}

// ---- C ABI (include/intel_hip.h) -----------------------------------------------------------------------------------------------------
#include "../../include/intel_hip.h"

extern "C" int intel_awelv_forward(int B, int L, int K, int H, const float* uid_table, long long users, const float* model_table,
                                   const int* u_id, const float* scores, float* w, float* weights, float* ens_score, void* stream) {
  INTEL_CHECK_ARG(uid_table && model_table && u_id && scores && w && weights && ens_score, "awelv_forward: null tensor");
  return launch_awelv_fwd(B, L, K, H, uid_table, users, model_table, u_id, scores, w, weights, ens_score, (hipStream_t)stream);
}

extern "C" size_t intel_awelv_backward_workspace_bytes(int B, int K, int H) { return awelv_bwd_ws_bytes(B, K, H); }

extern "C" int intel_awelv_backward(int B, int L, int K, int H, const float* uid_table, long long users, const float* model_table,
                                    const int* u_id, const float* scores, const float* w, const float* d_ens, const float* d_weights,
                                    float* d_uid_table, unsigned char* row_flags, float* d_model_table, void* workspace, void* stream) {
  INTEL_CHECK_ARG(uid_table && model_table && u_id && scores && w && d_ens && d_uid_table && d_model_table && workspace,
                  "awelv_backward: null tensor / workspace");
  return launch_awelv_bwd(B, L, K, H, uid_table, users, model_table, u_id, scores, w, d_ens, d_weights, d_uid_table, row_flags, d_model_table,
                          workspace, (hipStream_t)stream);
}
