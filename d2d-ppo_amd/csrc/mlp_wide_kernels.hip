// Wide MLP learners on gfx950: hidden sizes 65..128 with 33..64 network inputs (obs_dim 32..63 plus the bias
// column), the shapes the register-resident kernels of policy_kernels.hip / update_kernels.hip do not take
// (their split weight fragments at (KC, HT) = (2, 8) do not fit the register file).
//
//   d2d_policy_mlp_wide_step   the behaviour-policy slot     (semantics of d2d_policy_mlp_step)
//   d2d_ppo_actor_grad_wide    clipped-surrogate gradients   (semantics of d2d_ppo_actor_grad)
//   d2d_ppo_critic_grad_wide   squared-error gradients       (semantics of d2d_ppo_critic_grad_values)
//
// Design: the weights live in LDS, shared by the four waves of a workgroup (one agent per workgroup), as fp32
// images W1' [128][64] with the layer-1 bias in input column F and zeros past F / past H; every product runs on
// v_mfma_f32_16x16x4_f32, an fp32 fmaf chain -- torch fp32's accuracy with no operand split, and 4 registers per
// 16x16 accumulator.  A wave owns 16-sample tiles; its input tile X [16][64] (column F = 1) is staged in the wave's
// own LDS slice from fp32 rows or from the compact obs record (64-byte rows here), so both formats feed the same
// arithmetic and give the same bits on integer inputs.  Operand conventions (lane = (g, i), g = lane >> 4):
// A holds row i at k-slot g, B column i at k-slot g, the accumulator column i at rows 4g .. 4g + 3.
//   forward   H^T = W1' . X^T      (hidden on rows, sample on i); the accumulator is the B operand of
//             Z^T = W2 . relu(H^T) with the k order permuted (step (t, r) <-> hidden 16t + 4g + r)
//   backward  dH^T = W2^T . dZ^T   (dZ from ppo_dz, again consumed in place: step r <-> action 4g + r),
//             dW1' = dA^T . X and dW2 = dZ^T . h contract the samples: dA, h and dZ go through the wave's LDS
//             slice as [sample][.] and come back sample-on-k.
// Sums: a wave adds its tiles in MFMA accumulators, writes one partial per (wave, agent); wide_reduce_kernel adds
// the partials in index order.  No atomics: a repeated launch gives the same bits.
#include <algorithm>
#include <cmath>

#include "policy_split.h"
#include "ppo_epilogue.h"

namespace d2d {

constexpr int kWideHP = 128;  // hidden rows of a W1' image (HT = 8 tiles; rows past H are zero)
constexpr int kWideXS = 68;   // floats per row of W1' / X: 64 inputs + 4 (b128 reads of 16 lanes hit distinct banks)
constexpr int kWideHS = 132;  // floats per row of [.][hidden] tiles: 128 + 4
constexpr int kWideZS = 20;   // floats per row of the dZ tile [sample][16 actions] + 4
constexpr int kWideHT = kWideHP / 16;

__device__ __forceinline__ f32x4 mfma_f32(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// W1' image of one agent by the whole workgroup: [hid][col] = W1[hid][col] (col < F), b1[hid] (col == F), else 0
__device__ __forceinline__ void fill_w1_image(float* img, const float* __restrict__ W1, const float* __restrict__ b1,
                                              int H, int F) {
  for (int idx = threadIdx.x; idx < kWideHP * 64; idx += 256) {
    const int row = idx >> 6, col = idx & 63;
    float v = 0.f;
    if (row < H) v = col < F ? W1[(size_t)row * F + col] : col == F ? b1[row] : 0.f;
    img[row * kWideXS + col] = v;
  }
}

// X tile of one wave: row m = input row (row0 + m * rstride) for m < nvalid, zeros past it; column `lane`.
// fp32 rows: columns < F from memory, column F := 1, the rest 0.  Record rows (64 bytes): every byte is an input
// (the record holds the 1 at column F and zeros past it); `sbit`: this lane's column is int8 for this agent.
__device__ __forceinline__ void stage_x_tile(float* xs, const float* __restrict__ obs, const uint8_t* __restrict__ rec,
                                             bool sbit, int64_t row0, int64_t rstride, int nvalid, int F, int lane) {
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const bool ok = m < nvalid;
    const int64_t row = row0 + m * rstride;
    float v = 0.f;
    if (rec) {
      if (ok) {
        const uint32_t b = rec[row * 64 + lane];
        v = sbit ? (float)(int)(int8_t)b : (float)b;
      }
    } else {
      if (ok && lane < F) v = obs[row * F + lane];
      if (ok && lane == F) v = 1.f;
    }
    xs[m * kWideXS + lane] = v;
  }
}

// layer 1 of one tile, transposed: acc[t][r] = pre-activation of hidden 16t + 4g + r for sample i
__device__ __forceinline__ void wide_layer1(f32x4 (&acc)[kWideHT], const float* img, const f32x4 (&xb)[4], int g, int i) {
#pragma unroll
  for (int t = 0; t < kWideHT; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 wa = ld4(&img[(16 * t + i) * kWideXS + 16 * q + 4 * g]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t] = mfma_f32(wa[j], xb[q][j], acc[t]);
    }
  }
}

// ------------------------------------------------------------------------------------------ policy slot
template <int KIND, bool CRITIC>
__global__ __launch_bounds__(256) void policy_wide_kernel(MlpArgs a) {
  __shared__ __attribute__((aligned(16))) float w1s[kWideHP * kWideXS];
  __shared__ __attribute__((aligned(16))) float v1s[CRITIC ? kWideHP * kWideXS : 4];
  __shared__ __attribute__((aligned(16))) float xs_all[4][16 * kWideXS];
  const bool sampling = !a.forced && !a.deterministic;
  const uint32_t rng = (sampling && a.rng_off) ? a.rng_step + *a.rng_off : a.rng_step;
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int N = a.N, F = a.F, H = a.H, A = a.A;

  fill_w1_image(w1s, a.w1 + (size_t)k * H * F, a.b1 + (size_t)k * H, H, F);
  if constexpr (CRITIC) fill_w1_image(v1s, a.v1 + (size_t)k * H * F, a.c1 + (size_t)k * H, H, F);
  // layer-2 fragments in registers: actor A operand (row = action i, k-slot g <-> hidden 16t + 4g + r)
  float w2f[kWideHT][4], v2f[kWideHT][4];
#pragma unroll
  for (int t = 0; t < kWideHT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int hid = 16 * t + 4 * g + r;
      w2f[t][r] = (hid < H && i < A) ? a.w2[((size_t)k * A + i) * H + hid] : 0.f;
      v2f[t][r] = (CRITIC && hid < H) ? a.v2[(size_t)k * H + hid] : 0.f;
    }
  f32x4 b2i;
#pragma unroll
  for (int r = 0; r < 4; ++r) b2i[r] = 4 * g + r < A ? a.b2[(size_t)k * A + 4 * g + r] : 0.f;
  const float c2 = CRITIC ? a.c2[k] : 0.f;
  const bool sbit = a.rec ? ((a.sgn[(size_t)k * 2 + (lane >> 5)] >> (lane & 31)) & 1u) != 0 : false;
  __syncthreads();

  float* xs = xs_all[wave];
  const int tiles = a.envs_per_wave / 16;
  const int wave_env0 = (blockIdx.y * 4 + wave) * a.envs_per_wave;
  for (int tt = 0; tt < tiles; ++tt) {
    const int e0 = wave_env0 + tt * 16;
    if (e0 >= a.E) break;  // wave-uniform
    stage_x_tile(xs, a.obs, a.rec, sbit, (int64_t)e0 * N + k, N, min(16, a.E - e0), F, lane);
    lds_order();
    f32x4 xb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) xb[q] = ld4(&xs[i * kWideXS + 16 * q + 4 * g]);
    f32x4 h[kWideHT];
    wide_layer1(h, w1s, xb, g, i);
    f32x4 lg = b2i;
#pragma unroll
    for (int t = 0; t < kWideHT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) lg = mfma_f32(w2f[t][r], relu(h[t][r]), lg);
    float value = 0.f;
    if constexpr (CRITIC) {
      wide_layer1(h, v1s, xb, g, i);
      float pv = 0.f;
#pragma unroll
      for (int t = 0; t < kWideHT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) pv = fmaf(relu(h[t][r]), v2f[t][r], pv);
      value = group_sum(pv) + c2;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) lg[r] *= kLog2e;
    const int env = e0 + i;
    policy_epilogue<KIND, CRITIC, false, kModeRuntime>(a, lg, value, env, env < a.E, k, g, rng);
    lds_order();  // the tile's reads of xs are done before the next tile is staged
  }
}

// ------------------------------------------------------------------------------------------ update
struct WideUpdArgs {
  int T, E, N, F, H, A, kind, mask_bytes;
  int tiles_per_t, n_tiles, G, P;
  float inv_A, clip_lo, clip_hi, beta, scale;
  const float *w1, *b1, *w2, *b2;
  const float* obs;       // [T][E][N][F]
  const uint8_t* rec;     // [T][E][N][64]
  const uint32_t* sgn;    // [N][2]
  const void* actions;    // [T][E][N]
  const float* logp_old;  // actor: element (t, e, k) at t*st[0] + e*st[1] + k*st[2]
  const float* weight;    // actor: advantage / M; critic: return target
  int64_t lo_st[3], w_st[3];
  float* partial;         // [4 G][N][P]: one per wave
  float* vout;            // critic: NULL or V of sample (t, e, k) at t*v_st[0] + e*v_st[1] + k*v_st[2]
  int64_t v_st[3];
};

// Gradients of one agent's loss over the 16-sample tiles of this wave.  CRITIC: the Value net (A = 1, row 0 of the
// layer-2 operands), dZ = 2 scale (V - R).
template <int KIND, bool CRITIC>
__global__ __launch_bounds__(256) void ppo_wide_grad_kernel(WideUpdArgs a) {
  __shared__ __attribute__((aligned(16))) float w1s[kWideHP * kWideXS];
  __shared__ __attribute__((aligned(16))) float w2s[16 * kWideHS];      // [action][hidden], zero past A / H
  __shared__ __attribute__((aligned(16))) float xs_all[4][16 * kWideXS];
  __shared__ __attribute__((aligned(16))) float hs_all[4][16 * kWideHS];  // relu(h)  [sample][hidden]
  __shared__ __attribute__((aligned(16))) float da_all[4][16 * kWideHS];  // dL/dpre  [sample][hidden]
  __shared__ __attribute__((aligned(16))) float dz_all[4][16 * kWideZS];  // dL/dz    [sample][action]
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int N = a.N, F = a.F, H = a.H, A = a.A, E = a.E;

  fill_w1_image(w1s, a.w1 + (size_t)k * H * F, a.b1 + (size_t)k * H, H, F);
  for (int idx = threadIdx.x; idx < 16 * kWideHP; idx += 256) {
    const int act = idx >> 7, hid = idx & 127;
    w2s[act * kWideHS + hid] = (act < A && hid < H) ? a.w2[((size_t)k * A + act) * H + hid] : 0.f;
  }
  f32x4 b2i;
#pragma unroll
  for (int r = 0; r < 4; ++r) b2i[r] = 4 * g + r < A ? a.b2[(size_t)k * A + 4 * g + r] : 0.f;
  const bool sbit = a.rec ? ((a.sgn[(size_t)k * 2 + (lane >> 5)] >> (lane & 31)) & 1u) != 0 : false;
  __syncthreads();

  float *xs = xs_all[wave], *hs = hs_all[wave], *das = da_all[wave], *dzs = dz_all[wave];
  f32x4 gw1[kWideHT][4], gw2[kWideHT];
#pragma unroll
  for (int t = 0; t < kWideHT; ++t) {
    gw2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) gw1[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 gb2 = {0.f, 0.f, 0.f, 0.f};
  float s0 = 0.f, s1 = 0.f;  // actor: sum min-surrogate, sum entropy; critic: sum (V - R)^2, 0

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
      if constexpr (!CRITIC) {
        lo = a.logp_old[t * a.lo_st[0] + e * a.lo_st[1] + k * a.lo_st[2]];
        act = KIND == 0 ? load_mask(a.actions, (size_t)cell, a.mask_bytes)
                        : (uint32_t) reinterpret_cast<const uint8_t*>(a.actions)[cell];
      }
    }
    stage_x_tile(xs, a.obs, a.rec, sbit, ((int64_t)t * E + e0) * N + k, N, min(16, E - e0), F, lane);
    lds_order();
    f32x4 xb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) xb[q] = ld4(&xs[i * kWideXS + 16 * q + 4 * g]);
    f32x4 pre[kWideHT];
    wide_layer1(pre, w1s, xb, g, i);
    // layer 2: z[r] = logit of action 4g + r (critic: V in row 0) for sample i
    f32x4 z = b2i;
#pragma unroll
    for (int t2 = 0; t2 < kWideHT; ++t2) {
      const f32x4 wa = ld4(&w2s[i * kWideHS + 16 * t2 + 4 * g]);
#pragma unroll
      for (int r = 0; r < 4; ++r) z = mfma_f32(wa[r], relu(pre[t2][r]), z);
    }
    f32x4 dz;
    if constexpr (CRITIC) {
      const float diff = z[0] - W;
      const bool mine = ok && g == 0;
      dz = f32x4{mine ? 2.f * a.scale * diff : 0.f, 0.f, 0.f, 0.f};
      s0 += mine ? diff * diff : 0.f;
      if (mine && a.vout) a.vout[t * a.v_st[0] + e * a.v_st[1] + k * a.v_st[2]] = z[0];
    } else {
      dz = ppo_dz<KIND, false>(a, z, act, lo, W, ok, g, s0, s1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) gb2[r] += dz[r];
    // dH^T = W2^T . dZ^T (row = hidden 16t + i, k-slot g at step r <-> action 4g + r), masked by relu
#pragma unroll
    for (int t2 = 0; t2 < kWideHT; ++t2) {
      f32x4 dh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) dh = mfma_f32(w2s[(4 * g + r) * kWideHS + 16 * t2 + i], dz[r], dh);
      f32x4 hv, dv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        hv[r] = relu(pre[t2][r]);
        dv[r] = pre[t2][r] > 0.f ? dh[r] : 0.f;
      }
      st4(&hs[i * kWideHS + 16 * t2 + 4 * g], hv);
      st4(&das[i * kWideHS + 16 * t2 + 4 * g], dv);
    }
    st4(&dzs[i * kWideZS + 4 * g], dz);
    lds_order();
    // dW1' += dA^T . X and dW2 += dZ^T . h over the tile's samples (k-slot g at step s <-> sample 4s + g)
    float xk[4][4], zk[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      zk[s] = dzs[(4 * s + g) * kWideZS + i];
#pragma unroll
      for (int q = 0; q < 4; ++q) xk[s][q] = xs[(4 * s + g) * kWideXS + 16 * q + i];
    }
#pragma unroll
    for (int t2 = 0; t2 < kWideHT; ++t2) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float dak = das[(4 * s + g) * kWideHS + 16 * t2 + i];
        const float hk = hs[(4 * s + g) * kWideHS + 16 * t2 + i];
#pragma unroll
        for (int q = 0; q < 4; ++q) gw1[t2][q] = mfma_f32(dak, xk[s][q], gw1[t2][q]);
        gw2[t2] = mfma_f32(zk[s], hk, gw2[t2]);
      }
    }
    lds_order();  // the tile's LDS reads are done before the next tile is staged
  }

  // this wave's partial [P]: w1 [H][F] | b1 [H] | w2 [A][H] | b2 [A] | stats [2]
  float* out = a.partial + ((size_t)(blockIdx.y * 4 + wave) * N + k) * a.P;
  const int OB1 = H * F, OW2 = OB1 + H, OB2 = OW2 + A * H, OST = OB2 + A;
#pragma unroll
  for (int t = 0; t < kWideHT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int hid = 16 * t + 4 * g + r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = 16 * q + i;
        if (hid < H && col < F) out[hid * F + col] = gw1[t][q][r];
        else if (hid < H && col == F) out[OB1 + hid] = gw1[t][q][r];
      }
      const int act = 4 * g + r, hcol = 16 * t + i;
      if (act < A && hcol < H) out[OW2 + act * H + hcol] = gw2[t][r];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float v = row_sum16(gb2[r]);
    if (i == 0 && 4 * g + r < A) out[OB2 + 4 * g + r] = v;
  }
  // the stats were accumulated by the lanes of group 0 (ppo_dz: ga == 0)
  const float t0 = row_sum16(s0), t1 = row_sum16(s1);
  if (lane == 0) {
    out[OST] = t0;
    out[OST + 1] = CRITIC ? 0.f : t1;
  }
}

// Fixed-order sum of the W wave partials of every (agent, parameter) -> gradient tensors
__global__ void wide_reduce_kernel(const float* __restrict__ partial, int W, int N, int P, int H, int F, int A,
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

static const char kEnvelope[] = "the wide MLP kernels take 64 < hidden <= 128 with 32 < obs_dim + 1 <= 64 and n_out <= 16";

// the wide envelope (n_out < 0: not checked, the critic)
static int check_wide_shape(const char* fn, const d2d_mlp_desc* d, bool actor) {
  if (d->hidden <= 64 || d->hidden > 128 || d->obs_dim + 1 <= 32 || d->obs_dim + 1 > 64 ||
      (actor && (d->n_out < 1 || d->n_out > 16))) {
    d2d_set_error("%s: hidden=%d obs_dim=%d n_out=%d: %s", fn, d->hidden, d->obs_dim, d->n_out, kEnvelope);
    return D2D_EUNSUPPORTED;
  }
  return D2D_OK;
}

extern "C" int d2d_policy_mlp_wide_step(const d2d_mlp_desc* d, const void* obs, const void* forced, uint32_t rng_step,
                                        int32_t deterministic, void* actions, float* logp, float* value,
                                        void* stream) {
  // actions may be NULL in forced mode only (the log-probs of given actions: nothing else to write)
  if (!d || !obs || (!actions && !forced) || !logp || !d->w1 || !d->b1 || !d->w2 || !d->b2) {
    d2d_set_error("d2d_policy_mlp_wide_step: NULL argument");
    return D2D_EINVAL;
  }
  if (d->kind != 0 && d->kind != 1) { d2d_set_error("kind must be 0 (Bernoulli) or 1 (Categorical)"); return D2D_EINVAL; }
  if (d->n_envs < 0 || d->n_agents < 0) { d2d_set_error("d2d_policy_mlp_wide_step: negative size"); return D2D_EINVAL; }
  if (const int rc = check_wide_shape("d2d_policy_mlp_wide_step", d, true)) return rc;
  if (d->v1 && (!d->c1 || !d->v2 || !d->c2)) { d2d_set_error("critic needs v1, c1, v2, c2"); return D2D_EINVAL; }
  MlpArgs a{};
  a.E = d->n_envs; a.N = d->n_agents; a.F = d->obs_dim; a.H = d->hidden; a.A = d->n_out; a.kind = d->kind;
  a.deterministic = deterministic ? 1 : 0;
  a.inv_A = 1.f / (float)a.A;
  if (const int rc = obs_format_args(d->obs_format, d->obs_signed, d->obs_dim, obs, a.obs, a.rec, a.sgn)) return rc;
  // 64 envs (4 tiles) per wave amortise the workgroup's weight images; a small batch takes fewer, down to one
  // tile, so that about 1024 waves (one per SIMD) share it
  a.envs_per_wave = 64;
  while (a.envs_per_wave > 16 && (int64_t)a.E * a.N / a.envs_per_wave < 1024) a.envs_per_wave >>= 1;
  a.rng_step = rng_step; a.rng_off = d->rng_offset; a.seed = d->seed; a.env_base = d->env_base;
  a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2; a.b2 = d->b2;
  // the critic runs only where its value is stored
  const bool critic = d->v1 != nullptr && value != nullptr;
  if (critic) { a.v1 = d->v1; a.c1 = d->c1; a.v2 = d->v2; a.c2 = d->c2; }
  a.forced = forced; a.act_out = actions; a.logp_out = logp; a.value_out = value;
  a.mask_bytes = a.A <= 8 ? 1 : 2;
  if (a.E == 0 || a.N == 0) return D2D_OK;
  const int64_t gy = ((int64_t)a.E + 4 * a.envs_per_wave - 1) / (4 * a.envs_per_wave);
  if (gy > 65535) { d2d_set_error("d2d_policy_mlp_wide_step: n_envs=%d too large", a.E); return D2D_EUNSUPPORTED; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a.N, (unsigned)gy), block(256);
  if (a.kind == 0 && critic) hipLaunchKernelGGL((policy_wide_kernel<0, true>), grid, block, 0, s, a);
  else if (a.kind == 0) hipLaunchKernelGGL((policy_wide_kernel<0, false>), grid, block, 0, s, a);
  else if (critic) hipLaunchKernelGGL((policy_wide_kernel<1, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((policy_wide_kernel<1, false>), grid, block, 0, s, a);
  D2D_CHECK_HIP(hipGetLastError());
  return D2D_OK;
}

// Workgroups per agent of the update kernels (each of 4 waves; wave w of the 4 G takes the 16-sample tiles
// w, w + 4 G, ...): one wave per tile while about 256 workgroups -- one per CU -- cover all agents, then more
// tiles per wave, at most 256 of them (the fp32 accumulation chain of a wave), and grid.y <= 65535.
static int wide_blocks(int N, int64_t n_tiles) {
  int64_t G = std::min<int64_t>((n_tiles + 3) / 4, std::max<int64_t>(1, 256 / std::max(1, N)));
  G = std::max<int64_t>(G, (n_tiles + 4 * 256 - 1) / (4 * 256));
  return (int)std::max<int64_t>(1, std::min<int64_t>(G, 65535));
}
static int64_t wide_tiles(int T, int E) { return (int64_t)T * ((E + 15) / 16); }

extern "C" int64_t d2d_ppo_wide_workspace(int32_t n_agents, int32_t T, int32_t n_envs, int32_t obs_dim, int32_t hidden,
                                          int32_t n_out) {
  if (n_agents <= 0 || T <= 0 || n_envs <= 0) return 0;
  const int G = wide_blocks(n_agents, wide_tiles(T, n_envs));
  const int64_t P = (int64_t)hidden * obs_dim + hidden + (int64_t)n_out * hidden + n_out + 2;
  return 4 * (int64_t)G * n_agents * P;
}

static int64_t wide_extent_ok(const int64_t* st) { return st[0] >= 0 && st[1] >= 0 && st[2] >= 0; }

static int check_wide_update(const char* fn, const d2d_mlp_desc* d, int T, const void* obs, float* gw1, float* gb1,
                             float* gw2, float* gb2, float* workspace, int64_t ws, bool critic, WideUpdArgs& a) {
  if (!d || !obs || !d->w1 || !d->b1 || !d->w2 || !d->b2 || !gw1 || !gb1 || !gw2 || !gb2) {
    d2d_set_error("%s: NULL argument", fn);
    return D2D_EINVAL;
  }
  if (T < 0 || d->n_envs < 0 || d->n_agents < 0) { d2d_set_error("%s: negative size", fn); return D2D_EINVAL; }
  if (!critic && d->kind != 0 && d->kind != 1) { d2d_set_error("kind must be 0 or 1"); return D2D_EINVAL; }
  if (const int rc = check_wide_shape(fn, d, !critic)) return rc;
  a = WideUpdArgs{};
  if (const int rc = obs_format_args(d->obs_format, d->obs_signed, d->obs_dim, obs, a.obs, a.rec, a.sgn)) return rc;
  a.T = T; a.E = d->n_envs; a.N = d->n_agents; a.F = d->obs_dim; a.H = d->hidden;
  a.A = critic ? 1 : d->n_out; a.kind = d->kind;
  a.mask_bytes = a.A <= 8 ? 1 : 2;
  a.tiles_per_t = (a.E + 15) / 16;
  const int64_t tiles = wide_tiles(T, a.E);
  if (tiles > 0x7FFFFFFF) { d2d_set_error("%s: too many samples", fn); return D2D_EUNSUPPORTED; }
  a.n_tiles = (int)tiles;
  a.G = wide_blocks(a.N, tiles);
  a.P = a.H * a.F + a.H + a.A * a.H + a.A + 2;
  a.inv_A = 1.f / (float)a.A;
  a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2; a.b2 = d->b2;
  const int64_t need = d2d_ppo_wide_workspace(a.N, T, a.E, a.F, a.H, a.A);
  if (need > 0 && (!workspace || ws < need)) {
    d2d_set_error("%s: workspace %lld < %lld floats", fn, (long long)(workspace ? ws : 0), (long long)need);
    return D2D_EINVAL;
  }
  a.partial = workspace;
  return D2D_OK;
}

static int wide_zero_outputs(const WideUpdArgs& a, float* gw1, float* gb1, float* gw2, float* gb2, float* stats,
                             hipStream_t s) {
  const size_t N = (size_t)a.N;
  D2D_CHECK_HIP(hipMemsetAsync(gw1, 0, sizeof(float) * N * a.H * a.F, s));
  D2D_CHECK_HIP(hipMemsetAsync(gb1, 0, sizeof(float) * N * a.H, s));
  D2D_CHECK_HIP(hipMemsetAsync(gw2, 0, sizeof(float) * N * a.A * a.H, s));
  D2D_CHECK_HIP(hipMemsetAsync(gb2, 0, sizeof(float) * N * a.A, s));
  if (stats) D2D_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(float) * N * 2, s));
  return D2D_OK;
}

static int wide_reduce(const WideUpdArgs& a, float* gw1, float* gb1, float* gw2, float* gb2, float* stats,
                       hipStream_t s) {
  const int64_t n = (int64_t)a.N * a.P;
  hipLaunchKernelGGL(wide_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.partial, 4 * a.G, a.N,
                     a.P, a.H, a.F, a.A, gw1, gb1, gw2, gb2, stats);
  D2D_CHECK_HIP(hipGetLastError());
  return D2D_OK;
}

extern "C" int d2d_ppo_actor_grad_wide(const d2d_mlp_desc* d, int32_t T, const void* obs, const void* actions,
                                       const float* logp_old, const int64_t* logp_strides, const float* weight,
                                       const int64_t* weight_strides, float clip, float beta, float scale, float* gw1,
                                       float* gb1, float* gw2, float* gb2, float* stats, float* workspace,
                                       int64_t workspace_floats, void* stream) {
  WideUpdArgs a;
  if (!actions || !logp_old || !logp_strides || !weight || !weight_strides) {
    d2d_set_error("d2d_ppo_actor_grad_wide: NULL argument");
    return D2D_EINVAL;
  }
  if (!wide_extent_ok(logp_strides) || !wide_extent_ok(weight_strides)) {
    d2d_set_error("d2d_ppo_actor_grad_wide: negative logp / weight strides");
    return D2D_EINVAL;
  }
  if (const int rc = check_wide_update("d2d_ppo_actor_grad_wide", d, T, obs, gw1, gb1, gw2, gb2, workspace,
                                       workspace_floats, false, a))
    return rc;
  a.actions = actions; a.logp_old = logp_old; a.weight = weight;
  for (int q = 0; q < 3; ++q) { a.lo_st[q] = logp_strides[q]; a.w_st[q] = weight_strides[q]; }
  a.clip_lo = 1.f - clip; a.clip_hi = 1.f + clip; a.beta = beta; a.scale = scale;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a.N == 0) return D2D_OK;
  if (a.n_tiles == 0) return wide_zero_outputs(a, gw1, gb1, gw2, gb2, stats, s);
  const dim3 grid(a.N, a.G), block(256);
  if (a.kind == 0) hipLaunchKernelGGL((ppo_wide_grad_kernel<0, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((ppo_wide_grad_kernel<1, false>), grid, block, 0, s, a);
  D2D_CHECK_HIP(hipGetLastError());
  return wide_reduce(a, gw1, gb1, gw2, gb2, stats, s);
}

extern "C" int d2d_ppo_critic_grad_wide(const d2d_mlp_desc* d, int32_t T, const void* obs, const float* returns,
                                        const int64_t* return_strides, float scale, float* gw1, float* gb1,
                                        float* gw2, float* gb2, float* stats, float* workspace,
                                        int64_t workspace_floats, float* values, const int64_t* values_strides,
                                        void* stream) {
  WideUpdArgs a;
  if (!returns || !return_strides) { d2d_set_error("d2d_ppo_critic_grad_wide: NULL argument"); return D2D_EINVAL; }
  if (values && !values_strides) { d2d_set_error("d2d_ppo_critic_grad_wide: values without strides"); return D2D_EINVAL; }
  if (!wide_extent_ok(return_strides) || (values && !wide_extent_ok(values_strides))) {
    d2d_set_error("d2d_ppo_critic_grad_wide: negative return / value strides");
    return D2D_EINVAL;
  }
  if (const int rc = check_wide_update("d2d_ppo_critic_grad_wide", d, T, obs, gw1, gb1, gw2, gb2, workspace,
                                       workspace_floats, true, a))
    return rc;
  a.weight = returns;
  for (int q = 0; q < 3; ++q) a.w_st[q] = return_strides[q];
  a.vout = values;
  if (values) for (int q = 0; q < 3; ++q) a.v_st[q] = values_strides[q];
  a.scale = scale;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a.N == 0) return D2D_OK;
  if (a.n_tiles == 0) return wide_zero_outputs(a, gw1, gb1, gw2, gb2, stats, s);
  hipLaunchKernelGGL((ppo_wide_grad_kernel<0, true>), dim3(a.N, a.G), dim3(256), 0, s, a);
  D2D_CHECK_HIP(hipGetLastError());
  return wide_reduce(a, gw1, gb1, gw2, gb2, stats, s);
}
