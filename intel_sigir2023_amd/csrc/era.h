// Launchers of era.hip (internal): the ERA baseline's rank features and population fitness.
#pragma once
#include "common.h"

#define ERA_MAX_L 256        // items per list (4 per lane)
#define ERA_MAX_F 8          // features per item = 2 + K
#define ERA_MAX_H 64         // hidden width
#define ERA_MAX_HIDDEN 2     // hidden layers

// feat [B, L, 2 + K] = [p10, mAgr, psc_0 .. psc_{K-1}] per item, zeros from session_len on
int launch_era_features(int B, int L, int K, const float* scores, const int* slen, int window, float* feat, hipStream_t st);
// genes of one solution: per Linear weight [out, in] then bias [out]; the last Linear has out = 1
int era_genes(int F, int n_hidden, const int* hidden);
size_t era_fitness_ws_bytes(int P, int B);
// gain_sum[p] += sum_b NDCG@1 of solution p on session b; pred_out (optional) [P, B, L]
int launch_era_fitness(int P, int B, int L, int F, int n_hidden, const int* hidden, const float* pop, const float* feat, const int* ranking,
                       const int* slen, int width, double* gain_sum, float* pred_out, void* ws, hipStream_t st);
