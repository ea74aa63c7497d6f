// MLP learners with a categorical head of 17..32 ids on gfx950 (the ChannelSelectionEnv with 16..31 channels:
// xp_gamma.py's env has 16 channels, 17 ids, 24 inputs), the head the one-tile kernels of policy_kernels.hip /
// update_kernels.hip / mlp_wide_kernels.hip refuse (n_out <= 16).
//
//   d2d_policy_mlp_actions_step   the behaviour-policy slot     (semantics of d2d_policy_mlp_step, kind 1)
//   d2d_ppo_actor_grad_actions    clipped-surrogate gradients   (semantics of d2d_ppo_actor_grad, kind 1)
//   d2d_ppo_actions_workspace     floats of scratch of the gradient call
//
// Envelope: kind 1, 17 <= n_out <= 32, 1 <= hidden <= 128, obs_dim + 1 <= 64, fp32 rows (no env writes a compact
// record for a head this wide).  The per-agent iPPO critic does not depend on the action count: its update stays on the
// existing critic entry points; its rollout value is computed here beside the actor where the caller stores it.
//
// Design (that of mlp_wide_kernels.hip, which already fits every (F, H) of this envelope): one agent per workgroup, the
// layer-1 image W1' [128][64] as fp32 in LDS with b1 in column F and zeros past F / past H, every product on
// v_mfma_f32_16x16x4_f32, a wave owns 16-sample tiles whose input tile X [16][64] (column F = 1) is staged in the
// wave's own LDS slice.  Hidden tiles past H (wave-uniform) are skipped.  Operand conventions (lane = (g, i),
// g = lane >> 4): A holds row i at k-slot g, B column i at k-slot g, the accumulator column i at rows 4g .. 4g + 3.
//   forward   H^T = W1' . X^T; Z^T = W2 . relu(H^T) for TWO action tiles: tile t holds ids 16t + 4g + r (W2 rows past
//             A are zero), the layout policy_epilogue_cat2 / ppo_dz_cat2 take
//   backward  dH^T = W2^T . dZ^T over both tiles (step (t, r) <-> id 16t + 4g + r); dW1' = dA^T . X (8 x 4
//             accumulator tiles) and dW2 = dZ^T . h (2 x 8) contract the samples: dA, h and dZ [sample][32] go through
//             the wave's LDS slice and come back sample-on-k.
// Sums: a wave adds its tiles in MFMA accumulators and writes one partial per (wave, agent); actions_reduce_kernel
// adds the partials in index order.  No atomics: a repeated launch gives the same bits.
#include <algorithm>
#include <cmath>

#include "policy_epilogue.h"
#include "ppo_epilogue.h"

namespace d2d {

constexpr int kActHP = 128;  // hidden rows of a W1' image (8 tiles; rows past H are zero)
constexpr int kActXS = 68;   // floats per row of W1' / X: 64 inputs + 4 (b128 reads of 16 lanes hit distinct banks)
constexpr int kActHS = 132;  // floats per row of [.][hidden] tiles: 128 + 4
constexpr int kActZS = 36;   // floats per row of the dZ tile [sample][32 ids] + 4
constexpr int kActHT = kActHP / 16;
constexpr int kActAP = 32;   // ids of the two action tiles

__device__ __forceinline__ f32x4 act_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 act_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void act_st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// W1' image of one agent by the whole workgroup: [hid][col] = W1[hid][col] (col < F), b1[hid] (col == F), else 0
__device__ __forceinline__ void act_fill_w1(float* img, const float* __restrict__ W1, const float* __restrict__ b1,
                                            int H, int F) {
  for (int idx = threadIdx.x; idx < kActHP * 64; idx += 256) {
    const int row = idx >> 6, col = idx & 63;
    float v = 0.f;
    if (row < H) v = col < F ? W1[(size_t)row * F + col] : col == F ? b1[row] : 0.f;
    img[row * kActXS + col] = v;
  }
}

// X tile of one wave from fp32 rows: row m = input row (row0 + m * rstride) for m < nvalid, zeros past it; column
// `lane`: columns < F from memory, column F := 1, the rest 0
__device__ __forceinline__ void act_stage_x(float* xs, const float* __restrict__ obs, int64_t row0, int64_t rstride,
                                            int nvalid, int F, int lane) {
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const bool ok = m < nvalid;
    float v = 0.f;
    if (ok && lane < F) v = obs[(row0 + m * rstride) * F + lane];
    if (ok && lane == F) v = 1.f;
    xs[m * kActXS + lane] = v;
  }
}

// layer 1 of one tile, transposed: acc[t][r] = pre-activation of hidden 16t + 4g + r for sample i (t < nt; else 0)
__device__ __forceinline__ void act_layer1(f32x4 (&acc)[kActHT], const float* img, const f32x4 (&xb)[4], int nt, int g,
                                           int i) {
#pragma unroll
  for (int t = 0; t < kActHT; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t < nt) {  // wave-uniform
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 wa = act_ld4(&img[(16 * t + i) * kActXS + 16 * q + 4 * g]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t] = act_mfma(wa[j], xb[q][j], acc[t]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ policy slot
template <bool CRITIC>
__global__ __launch_bounds__(256) void policy_actions_kernel(MlpArgs a) {
  __shared__ __attribute__((aligned(16))) float w1s[kActHP * kActXS];
  __shared__ __attribute__((aligned(16))) float v1s[CRITIC ? kActHP * kActXS : 4];
  __shared__ __attribute__((aligned(16))) float xs_all[4][16 * kActXS];
  const bool sampling = !a.forced && !a.deterministic;
  const uint32_t rng = (sampling && a.rng_off) ? a.rng_step + *a.rng_off : a.rng_step;
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int N = a.N, F = a.F, H = a.H, A = a.A;
  const int nt = (H + 15) >> 4;

  act_fill_w1(w1s, a.w1 + (size_t)k * H * F, a.b1 + (size_t)k * H, H, F);
  if constexpr (CRITIC) act_fill_w1(v1s, a.v1 + (size_t)k * H * F, a.c1 + (size_t)k * H, H, F);
  // layer-2 fragments in registers: actor A operand of action tile ta (row = id 16 ta + i, k-slot g <-> hidden
  // 16t + 4g + r), zero past A / past H
  float w2f[2][kActHT][4], v2f[kActHT][4];
#pragma unroll
  for (int t = 0; t < kActHT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int hid = 16 * t + 4 * g + r;
#pragma unroll
      for (int ta = 0; ta < 2; ++ta)
        w2f[ta][t][r] = (hid < H && 16 * ta + i < A) ? a.w2[((size_t)k * A + 16 * ta + i) * H + hid] : 0.f;
      v2f[t][r] = (CRITIC && hid < H) ? a.v2[(size_t)k * H + hid] : 0.f;
    }
  f32x4 b2i[2];
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int r = 0; r < 4; ++r) b2i[ta][r] = 16 * ta + 4 * g + r < A ? a.b2[(size_t)k * A + 16 * ta + 4 * g + r] : 0.f;
  const float c2 = CRITIC ? a.c2[k] : 0.f;
  __syncthreads();

  float* xs = xs_all[wave];
  const int tiles = a.envs_per_wave / 16;
  const int wave_env0 = (blockIdx.y * 4 + wave) * a.envs_per_wave;
  for (int tt = 0; tt < tiles; ++tt) {
    const int e0 = wave_env0 + tt * 16;
    if (e0 >= a.E) break;  // wave-uniform
    act_stage_x(xs, a.obs, (int64_t)e0 * N + k, N, min(16, a.E - e0), F, lane);
    lds_order();
    f32x4 xb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) xb[q] = act_ld4(&xs[i * kActXS + 16 * q + 4 * g]);
    f32x4 h[kActHT];
    act_layer1(h, w1s, xb, nt, g, i);
    f32x4 lg[2] = {b2i[0], b2i[1]};
#pragma unroll
    for (int t = 0; t < kActHT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float hv = relu(h[t][r]);
          lg[0] = act_mfma(w2f[0][t][r], hv, lg[0]);
          lg[1] = act_mfma(w2f[1][t][r], hv, lg[1]);
        }
      }
    const int env = e0 + i;
    const bool env_ok = env < a.E;
    if constexpr (CRITIC) {
      // V as policy_wide_kernel computes it: per-lane dot product over the lane's hidden units, then the 4 groups
      act_layer1(h, v1s, xb, nt, g, i);
      float pv = 0.f;
#pragma unroll
      for (int t = 0; t < kActHT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) pv = fmaf(relu(h[t][r]), v2f[t][r], pv);
      const float value = group_sum(pv) + c2;
      if (env_ok && g == 0) a.value_out[(size_t)k * a.E + env] = value;
    }
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
      for (int r = 0; r < 4; ++r) lg[ta][r] *= kLog2e;
    policy_epilogue_cat2<kModeRuntime>(a, lg, env, env_ok, k, g, rng);
    lds_order();  // the tile's reads of xs are done before the next tile is staged
  }
}

// ------------------------------------------------------------------------------------------ update
struct ActUpdArgs {
  int T, E, N, F, H, A;
  int tiles_per_t, n_tiles, G, P;
  float clip_lo, clip_hi, beta, scale;
  const float *w1, *b1, *w2, *b2;
  const float* obs;        // [T][E][N][F]
  const uint8_t* actions;  // [T][E][N] ids
  const float* logp_old;   // element (t, e, k) at t*st[0] + e*st[1] + k*st[2]
  const float* weight;     // advantage / M
  int64_t lo_st[3], w_st[3];
  float* partial;          // [4 G][N][P]: one per wave
};

// Gradients of one agent's actor loss over the 16-sample tiles of this wave
__global__ __launch_bounds__(256) void ppo_actions_grad_kernel(ActUpdArgs a) {
  __shared__ __attribute__((aligned(16))) float w1s[kActHP * kActXS];
  __shared__ __attribute__((aligned(16))) float w2s[kActAP * kActHS];      // [id][hidden], zero past A / H
  __shared__ __attribute__((aligned(16))) float xs_all[4][16 * kActXS];
  __shared__ __attribute__((aligned(16))) float hs_all[4][16 * kActHS];  // relu(h)  [sample][hidden]
  __shared__ __attribute__((aligned(16))) float da_all[4][16 * kActHS];  // dL/dpre  [sample][hidden]
  __shared__ __attribute__((aligned(16))) float dz_all[4][16 * kActZS];  // dL/dz    [sample][id]
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int N = a.N, F = a.F, H = a.H, A = a.A, E = a.E;
  const int nt = (H + 15) >> 4;

  act_fill_w1(w1s, a.w1 + (size_t)k * H * F, a.b1 + (size_t)k * H, H, F);
  for (int idx = threadIdx.x; idx < kActAP * kActHP; idx += 256) {
    const int act = idx >> 7, hid = idx & 127;
    w2s[act * kActHS + hid] = (act < A && hid < H) ? a.w2[((size_t)k * A + act) * H + hid] : 0.f;
  }
  f32x4 b2i[2];
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int r = 0; r < 4; ++r) b2i[ta][r] = 16 * ta + 4 * g + r < A ? a.b2[(size_t)k * A + 16 * ta + 4 * g + r] : 0.f;
  __syncthreads();

  float *xs = xs_all[wave], *hs = hs_all[wave], *das = da_all[wave], *dzs = dz_all[wave];
  f32x4 gw1[kActHT][4], gw2[2][kActHT];
#pragma unroll
  for (int t = 0; t < kActHT; ++t) {
    gw2[0][t] = gw2[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) gw1[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 gb2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  float s0 = 0.f, s1 = 0.f;  // sum min-surrogate, sum entropy

  const int stride = 4 * a.G;
  for (int tile = blockIdx.y * 4 + wave; tile < a.n_tiles; tile += stride) {
    const int t = tile / a.tiles_per_t, e0 = (tile - t * a.tiles_per_t) * 16;
    const int e = e0 + i;
    const bool ok = e < E;
    const int64_t cell = ((int64_t)t * E + (ok ? e : 0)) * N + k;
    // per-sample scalars of this lane's sample
    uint32_t act = 0;
    float lo = 0.f, W = 0.f;
    if (ok) {
      W = a.weight[t * a.w_st[0] + e * a.w_st[1] + k * a.w_st[2]];
      lo = a.logp_old[t * a.lo_st[0] + e * a.lo_st[1] + k * a.lo_st[2]];
      act = (uint32_t)a.actions[cell];
    }
    act_stage_x(xs, a.obs, ((int64_t)t * E + e0) * N + k, N, min(16, E - e0), F, lane);
    lds_order();
    f32x4 xb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) xb[q] = act_ld4(&xs[i * kActXS + 16 * q + 4 * g]);
    f32x4 pre[kActHT];
    act_layer1(pre, w1s, xb, nt, g, i);
    // layer 2: z[ta][r] = logit of id 16 ta + 4g + r for sample i
    f32x4 z[2] = {b2i[0], b2i[1]};
#pragma unroll
    for (int t2 = 0; t2 < kActHT; ++t2)
      if (t2 < nt) {
        const f32x4 wa0 = act_ld4(&w2s[i * kActHS + 16 * t2 + 4 * g]);
        const f32x4 wa1 = act_ld4(&w2s[(16 + i) * kActHS + 16 * t2 + 4 * g]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float hv = relu(pre[t2][r]);
          z[0] = act_mfma(wa0[r], hv, z[0]);
          z[1] = act_mfma(wa1[r], hv, z[1]);
        }
      }
    f32x4 dz[2];
    ppo_dz_cat2(a, z, act, lo, W, ok, g, s0, s1, dz);
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
      for (int r = 0; r < 4; ++r) gb2[ta][r] += dz[ta][r];
    // dH^T = W2^T . dZ^T (row = hidden 16t + i, k-slot g at step (ta, r) <-> id 16 ta + 4g + r), masked by relu
#pragma unroll
    for (int t2 = 0; t2 < kActHT; ++t2)
      if (t2 < nt) {
        f32x4 dh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dh = act_mfma(w2s[(16 * ta + 4 * g + r) * kActHS + 16 * t2 + i], dz[ta][r], dh);
        f32x4 hv, dv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          hv[r] = relu(pre[t2][r]);
          dv[r] = pre[t2][r] > 0.f ? dh[r] : 0.f;
        }
        act_st4(&hs[i * kActHS + 16 * t2 + 4 * g], hv);
        act_st4(&das[i * kActHS + 16 * t2 + 4 * g], dv);
      }
    act_st4(&dzs[i * kActZS + 4 * g], dz[0]);
    act_st4(&dzs[i * kActZS + 16 + 4 * g], dz[1]);
    lds_order();
    // dW1' += dA^T . X and dW2 += dZ^T . h over the tile's samples (k-slot g at step s <-> sample 4s + g)
    // (samples outermost: one step's X and dZ operands live at a time beside the 48 accumulator tiles)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float zk0 = dzs[(4 * s + g) * kActZS + i], zk1 = dzs[(4 * s + g) * kActZS + 16 + i];
      float xk[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) xk[q] = xs[(4 * s + g) * kActXS + 16 * q + i];
#pragma unroll
      for (int t2 = 0; t2 < kActHT; ++t2)
        if (t2 < nt) {
          const float dak = das[(4 * s + g) * kActHS + 16 * t2 + i];
          const float hk = hs[(4 * s + g) * kActHS + 16 * t2 + i];
#pragma unroll
          for (int q = 0; q < 4; ++q) gw1[t2][q] = act_mfma(dak, xk[q], gw1[t2][q]);
          gw2[0][t2] = act_mfma(zk0, hk, gw2[0][t2]);
          gw2[1][t2] = act_mfma(zk1, hk, gw2[1][t2]);
        }
    }
    lds_order();  // the tile's LDS reads are done before the next tile is staged
  }

  // this wave's partial [P]: w1 [H][F] | b1 [H] | w2 [A][H] | b2 [A] | stats [2]
  float* out = a.partial + ((size_t)(blockIdx.y * 4 + wave) * N + k) * a.P;
  const int OB1 = H * F, OW2 = OB1 + H, OB2 = OW2 + A * H, OST = OB2 + A;
#pragma unroll
  for (int t = 0; t < kActHT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int hid = 16 * t + 4 * g + r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = 16 * q + i;
        if (hid < H && col < F) out[hid * F + col] = gw1[t][q][r];
        else if (hid < H && col == F) out[OB1 + hid] = gw1[t][q][r];
      }
      const int hcol = 16 * t + i;
#pragma unroll
      for (int ta = 0; ta < 2; ++ta) {
        const int act = 16 * ta + 4 * g + r;
        if (act < A && hcol < H) out[OW2 + act * H + hcol] = gw2[ta][t][r];
      }
    }
  }
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = row_sum16(gb2[ta][r]);
      const int act = 16 * ta + 4 * g + r;
      if (i == 0 && act < A) out[OB2 + act] = v;
    }
  // the stats were accumulated by the lanes of group 0 (ppo_dz_cat2: g == 0)
  const float t0 = row_sum16(s0), t1 = row_sum16(s1);
  if (lane == 0) {
    out[OST] = t0;
    out[OST + 1] = t1;
  }
}

// Fixed-order sum of the W wave partials of every (agent, parameter) -> gradient tensors
__global__ void actions_reduce_kernel(const float* __restrict__ partial, int W, int N, int P, int H, int F, int A,
                                      float* gw1, float* gb1, float* gw2, float* gb2, float* stats) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)N * P) return;
  const int k = (int)(idx / P), p = (int)(idx - (int64_t)k * P);
  float s = 0.f;
  for (int b = 0; b < W; ++b) s += partial[((size_t)b * N + k) * P + p];
  const int OB1 = H * F, OW2 = OB1 + H, OB2 = OW2 + A * H, OST = OB2 + A;
  if (p < OB1) gw1[(size_t)k * H * F + p] = s;
  else if (p < OW2) gb1[(size_t)k * H + (p - OB1)] = s;
  else if (p < OB2) gw2[(size_t)k * A * H + (p - OW2)] = s;
  else if (p < OST) gb2[(size_t)k * A + (p - OB2)] = s;
  else if (stats) stats[(size_t)k * 2 + (p - OST)] = s;
}

}  // namespace d2d

using namespace d2d;

static const char kActEnvelope[] =
    "the MLP actions kernels take the categorical head (kind 1) with 17 <= n_out <= 32, 1 <= hidden <= 128 and "
    "obs_dim + 1 <= 64 on fp32 rows (no compact record)";

// kind (0 / 1 checked by the caller), the shape and the obs format
static int check_actions_desc(const char* fn, const d2d_mlp_desc* d) {
  if (d->kind != 1 || d->n_out < 17 || d->n_out > 32 || d->hidden < 1 || d->hidden > 128 || d->obs_dim < 1 ||
      d->obs_dim + 1 > 64) {
    d2d_set_error("%s: kind=%d hidden=%d obs_dim=%d n_out=%d: %s", fn, d->kind, d->hidden, d->obs_dim, d->n_out,
                  kActEnvelope);
    return D2D_EUNSUPPORTED;
  }
  if (d->obs_format == D2D_OBS_U8) {
    d2d_set_error("%s: the compact obs record is not an input of this head (n_out=%d): %s", fn, d->n_out,
                  kActEnvelope);
    return D2D_EUNSUPPORTED;
  }
  if (d->obs_format != D2D_OBS_F32) { d2d_set_error("unknown obs_format %d", d->obs_format); return D2D_EINVAL; }
  return D2D_OK;
}

extern "C" int d2d_policy_mlp_actions_step(const d2d_mlp_desc* d, const void* obs, const void* forced,
                                           uint32_t rng_step, int32_t deterministic, void* actions, float* logp,
                                           float* value, void* stream) {
  // actions may be NULL in forced mode only (the log-probs of given ids: nothing else to write)
  if (!d || !obs || (!actions && !forced) || !logp || !d->w1 || !d->b1 || !d->w2 || !d->b2) {
    d2d_set_error("d2d_policy_mlp_actions_step: NULL argument");
    return D2D_EINVAL;
  }
  if (d->kind != 0 && d->kind != 1) { d2d_set_error("kind must be 0 (Bernoulli) or 1 (Categorical)"); return D2D_EINVAL; }
  if (d->n_envs < 0 || d->n_agents < 0) { d2d_set_error("d2d_policy_mlp_actions_step: negative size"); return D2D_EINVAL; }
  if (const int rc = check_actions_desc("d2d_policy_mlp_actions_step", d)) return rc;
  if (d->v1 && (!d->c1 || !d->v2 || !d->c2)) { d2d_set_error("critic needs v1, c1, v2, c2"); return D2D_EINVAL; }
  MlpArgs a{};
  a.E = d->n_envs; a.N = d->n_agents; a.F = d->obs_dim; a.H = d->hidden; a.A = d->n_out; a.kind = 1;
  a.deterministic = deterministic ? 1 : 0;
  a.inv_A = 1.f / (float)a.A;
  a.obs = static_cast<const float*>(obs);
  // 64 envs (4 tiles) per wave amortise the workgroup's weight images; a small batch takes fewer, down to one
  // tile, so that about 1024 waves (one per SIMD) share it.  Grid: (n_agents, ceil(n_envs / (4 envs_per_wave)))
  a.envs_per_wave = 64;
  while (a.envs_per_wave > 16 && (int64_t)a.E * a.N / a.envs_per_wave < 1024) a.envs_per_wave >>= 1;
  a.rng_step = rng_step; a.rng_off = d->rng_offset; a.seed = d->seed; a.env_base = d->env_base;
  a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2; a.b2 = d->b2;
  // the critic runs only where its value is stored
  const bool critic = d->v1 != nullptr && value != nullptr;
  if (critic) { a.v1 = d->v1; a.c1 = d->c1; a.v2 = d->v2; a.c2 = d->c2; }
  a.forced = forced; a.act_out = actions; a.logp_out = logp; a.value_out = critic ? value : nullptr;
  a.mask_bytes = 1;
  if (a.E == 0 || a.N == 0) return D2D_OK;
  const int64_t gy = ((int64_t)a.E + 4 * a.envs_per_wave - 1) / (4 * a.envs_per_wave);
  if (gy > 65535) { d2d_set_error("d2d_policy_mlp_actions_step: n_envs=%d too large", a.E); return D2D_EUNSUPPORTED; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a.N, (unsigned)gy), block(256);
  if (critic) hipLaunchKernelGGL((policy_actions_kernel<true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((policy_actions_kernel<false>), grid, block, 0, s, a);
  D2D_CHECK_HIP(hipGetLastError());
  return D2D_OK;
}

// Workgroups per agent of the gradient kernel (each of 4 waves; wave w of the 4 G takes the 16-sample tiles
// w, w + 4 G, ...): one wave per tile while about 256 workgroups -- one per CU -- cover all agents, then more
// tiles per wave, at most 256 of them (the fp32 accumulation chain of a wave), and grid.y <= 65535.
static int actions_blocks(int N, int64_t n_tiles) {
  int64_t G = std::min<int64_t>((n_tiles + 3) / 4, std::max<int64_t>(1, 256 / std::max(1, N)));
  G = std::max<int64_t>(G, (n_tiles + 4 * 256 - 1) / (4 * 256));
  return (int)std::max<int64_t>(1, std::min<int64_t>(G, 65535));
}
static int64_t actions_tiles(int T, int E) { return (int64_t)T * ((E + 15) / 16); }

// 4 G N P floats: one partial of P = H F + H + A H + A + 2 floats per (wave, agent)
extern "C" int64_t d2d_ppo_actions_workspace(int32_t n_agents, int32_t T, int32_t n_envs, int32_t obs_dim,
                                             int32_t hidden, int32_t n_out) {
  if (n_agents <= 0 || T <= 0 || n_envs <= 0) return 0;
  const int G = actions_blocks(n_agents, actions_tiles(T, n_envs));
  const int64_t P = (int64_t)hidden * obs_dim + hidden + (int64_t)n_out * hidden + n_out + 2;
  return 4 * (int64_t)G * n_agents * P;
}

extern "C" int d2d_ppo_actor_grad_actions(const d2d_mlp_desc* d, int32_t T, const void* obs, const void* actions,
                                          const float* logp_old, const int64_t* logp_strides, const float* weight,
                                          const int64_t* weight_strides, float clip, float beta, float scale,
                                          float* gw1, float* gb1, float* gw2, float* gb2, float* stats,
                                          float* workspace, int64_t workspace_floats, void* stream) {
  const char* fn = "d2d_ppo_actor_grad_actions";
  if (!d || !obs || !actions || !logp_old || !logp_strides || !weight || !weight_strides || !d->w1 || !d->b1 ||
      !d->w2 || !d->b2 || !gw1 || !gb1 || !gw2 || !gb2) {
    d2d_set_error("%s: NULL argument", fn);
    return D2D_EINVAL;
  }
  for (int q = 0; q < 3; ++q)
    if (logp_strides[q] < 0 || weight_strides[q] < 0) {
      d2d_set_error("%s: negative logp / weight strides", fn);
      return D2D_EINVAL;
    }
  if (T < 0 || d->n_envs < 0 || d->n_agents < 0) { d2d_set_error("%s: negative size", fn); return D2D_EINVAL; }
  if (d->kind != 0 && d->kind != 1) { d2d_set_error("kind must be 0 or 1"); return D2D_EINVAL; }
  if (const int rc = check_actions_desc(fn, d)) return rc;
  ActUpdArgs a{};
  a.T = T; a.E = d->n_envs; a.N = d->n_agents; a.F = d->obs_dim; a.H = d->hidden; a.A = d->n_out;
  a.tiles_per_t = (a.E + 15) / 16;
  const int64_t tiles = actions_tiles(T, a.E);
  if (tiles > 0x7FFFFFFF) { d2d_set_error("%s: too many samples", fn); return D2D_EUNSUPPORTED; }
  a.n_tiles = (int)tiles;
  a.G = actions_blocks(a.N, tiles);
  a.P = a.H * a.F + a.H + a.A * a.H + a.A + 2;
  a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2; a.b2 = d->b2;
  const int64_t need = d2d_ppo_actions_workspace(a.N, T, a.E, a.F, a.H, a.A);
  if (need > 0 && (!workspace || workspace_floats < need)) {
    d2d_set_error("%s: workspace %lld < %lld floats", fn, (long long)(workspace ? workspace_floats : 0),
                  (long long)need);
    return D2D_EINVAL;
  }
  a.partial = workspace;
  a.obs = static_cast<const float*>(obs);
  a.actions = static_cast<const uint8_t*>(actions); a.logp_old = logp_old; a.weight = weight;
  for (int q = 0; q < 3; ++q) { a.lo_st[q] = logp_strides[q]; a.w_st[q] = weight_strides[q]; }
  a.clip_lo = 1.f - clip; a.clip_hi = 1.f + clip; a.beta = beta; a.scale = scale;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a.N == 0) return D2D_OK;
  if (a.n_tiles == 0) {
    const size_t N = (size_t)a.N;
    D2D_CHECK_HIP(hipMemsetAsync(gw1, 0, sizeof(float) * N * a.H * a.F, s));
    D2D_CHECK_HIP(hipMemsetAsync(gb1, 0, sizeof(float) * N * a.H, s));
    D2D_CHECK_HIP(hipMemsetAsync(gw2, 0, sizeof(float) * N * a.A * a.H, s));
    D2D_CHECK_HIP(hipMemsetAsync(gb2, 0, sizeof(float) * N * a.A, s));
    if (stats) D2D_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(float) * N * 2, s));
    return D2D_OK;
  }
  hipLaunchKernelGGL(ppo_actions_grad_kernel, dim3(a.N, a.G), dim3(256), 0, s, a);
  D2D_CHECK_HIP(hipGetLastError());
  const int64_t n = (int64_t)a.N * a.P;
  hipLaunchKernelGGL(actions_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.partial, 4 * a.G,
                     a.N, a.P, a.H, a.F, a.A, gw1, gb1, gw2, gb2, stats);
  D2D_CHECK_HIP(hipGetLastError());
  return D2D_OK;
}
