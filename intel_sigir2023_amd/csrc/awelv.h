// Launchers of awelv.hip (internal): the aWELv baseline's per-user fusion weights, forward and backward.
#pragma once
#include "common.h"

#define AWELV_KMAX 16        // base rankers (= LOSS_KMAX of loss.hip)
#define AWELV_HMAX 256       // hidden size: one float4 per lane of a wave
#define AWELV_BWD_MAX_WG 64  // workgroups of the backward (4 sessions each per round): bounds its workspace

// w [B, K] = softmax_k(E[u_b] . M[k]); weights [B, L, K] = w repeated over l; ens [B, L] = sum_k w_k scores[b, l, k]
int launch_awelv_fwd(int B, int L, int K, int H, const float* uid_table, long long users, const float* model_table, const int* u_id,
                     const float* scores, float* w, float* weights, float* ens, hipStream_t st);
size_t awelv_bwd_ws_bytes(int B, int K, int H);
// d_uid_table [users, H] is ADDED into (float atomics), row_flags[u_b] = 1 (optional), d_model_table [K, H] is WRITTEN
int launch_awelv_bwd(int B, int L, int K, int H, const float* uid_table, long long users, const float* model_table, const int* u_id,
                     const float* scores, const float* w, const float* d_ens, const float* d_weights, float* d_uid_table,
                     unsigned char* row_flags, float* d_model_table, void* ws, hipStream_t st);
