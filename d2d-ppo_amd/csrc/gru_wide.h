// Host interface of the wide GRU path (gru_wide_kernels.hip): the PPO RNN module for 64 < hidden <= 128.
// The entry points of gru_kernels.hip check the desc and the buffers, then branch here on hidden > 64.
#pragma once
#include <cstdint>

#include "d2d_hip.h"

namespace d2d {

constexpr int kGruNarrowHidden = 64;   // gru_kernels.hip: register-resident vectors, LDS weight images
constexpr int kGruWideHidden = 128;    // gru_wide_kernels.hip: LDS vector images, L2-resident weights

// History budget of one d2d_gru_grad call on the wide path, in floats (2 GiB).  A PPO batch is T * E windows per
// agent and one (agent, 16-sample tile) keeps 16 L (5 HW + IW) floats of x, h and gate history (2.8 MB at
// L = 64, H = 128, F = 30), so the whole batch does not fit; d2d_gru_grad runs it in chunks of whole tiles.  One
// BPTT workgroup is one wave with 53 KB of LDS, three to a CU: 768 of them fill the 256 CUs.  At the largest
// shape the learners run (64 agents, L = 64, H = 128, F = 30) 2 GiB holds 12 tiles per agent = 768 workgroups; smaller
// shapes reach the whole batch or thousands of tiles first, and the buffer stays under 1 % of the 288 GB of HBM
// per net.
constexpr int64_t kGruWideBudgetFloats = (int64_t)1 << 29;

int64_t gru_wide_carry_floats(const d2d_gru_desc* d);
int gru_wide_policy(const d2d_gru_desc* d, int32_t T, const void* obs, int32_t slot0, int32_t n_slots, int32_t padded,
                    const void* forced, uint32_t rng_step, int32_t deterministic, void* actions, float* out,
                    float* hcarry, int32_t carry_in, void* stream);
int64_t gru_wide_grad_workspace(const d2d_gru_desc* d, int32_t T);
int gru_wide_grad(const d2d_gru_desc* d, int32_t T, const void* obs, const void* actions, const float* logp_old,
                  const int64_t* logp_strides, const float* weight, const int64_t* weight_strides, float clip,
                  float beta, float scale, float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_w1,
                  float* g_b1, float* g_w2, float* g_b2, float* stats, float* workspace, int64_t workspace_floats,
                  void* stream);

}  // namespace d2d
