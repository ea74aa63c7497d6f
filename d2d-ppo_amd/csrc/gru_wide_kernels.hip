// The PPO learners' GRU policies and GRU critic for hidden sizes 65..128 on gfx950: the behaviour policy / value
// of observation windows (d2d_policy_gru, d2d_policy_gru_carry) and PPO.train_step's gradients (d2d_gru_grad),
// entered from gru_kernels.hip's entry points where hidden > 64.
//
//   network: GRU(F, H) -> Linear(H, H) -> ReLU -> Linear(H, n_out) -> sigmoid (kind 0) / softmax (1) / none (2),
//   h0 = 0 per window, torch's GRU formula and gate order (gru_common.h:5-8); the parameters of StackedNets "rnn".
//
// The kernels of gru_kernels.hip keep every vector in registers and the weights as LDS images, which stops at H = 64
// (DESIGN 4.7).  Here the layout is iRDQN's (rdqn_kernels.hip, gru_l2_common.h): one 16-sample tile per wave and one
// wave per workgroup, v_mfma_f32_16x16x4_f32 on transposed layers, a run-time tile count HT = ceil(H / 16), vectors
// as LDS vector images, weight fragments from the L2-resident agent-stacked tensors, zeros past H, F and A.  Every
// product is exact fp32.  On top of that sit the PPO pieces the narrow path uses: windows rebuilt from the rollout
// buffer obs [T][E][N] by slot and episode position, policy_epilogue.h after the head (sampled / deterministic /
// forced actions, log-probs) and ppo_epilogue.h's ppo_dz (or the critic's MSE) as the loss gradient.
//
// d2d_gru_grad runs, per chunk of whole tiles (gru_wide.h: the history of a PPO batch does not fit memory at once),
// (1) gru_wide_bptt_kernel per (agent, tile): the padded window's forward keeping x, h and the gates in the caller's
// workspace, head, loss gradient, head backward and BPTT, which overwrites each step's gates with its pre-activation
// gradients; (2) gru_wide_wgrad_kernel, one wave per 16 x 16 tile of a gradient tensor: the sum over (step, sample)
// of the chunk in a fixed order, no atomics, added to the output in stream order after the first chunk.
#include <algorithm>

#include "gru_l2_common.h"
#include "gru_wide.h"
#include "policy_epilogue.h"
#include "ppo_epilogue.h"

namespace d2d {
namespace {

enum { kWideBernoulli = 0, kWideCategorical = 1, kWideValue = 2 };

struct WideArgs {
  int N, E, F, H, A, HT, IT;
  int vecF, vecH;              // 16-byte fragment loads of F-wide / H-wide rows
  int T, L, ep_len, kind, env_tiles;
  const float *w_ih, *w_hh, *b_ih, *b_hh, *w1, *b1, *w2, *b2;
  const float* obs;            // rollout buffer [T][E][N][F] (fp32 rows; else rec below)
  const uint8_t* rec;          // the compact record [T][E][N][RB] (D2D_OBS_U8) with
  const uint32_t* sgn;         // its int8-column masks [N][RB / 32]
  int RB;
  // policy kernel: tiles = slots [slot0, slot0 + n_slots) x env_tiles
  int slot0, n_slots, padded, carry_in;
  MlpArgs ep;                  // epilogue view: ep.E = n_slots * E (slot-major samples)
  float* value_out;            // kind 2: [N][n_slots * E]
  float* hcarry;               // [N][env_tiles][HT][64] f32x4: the final h image of every (agent, tile)
  // grad kernels: tiles [tile0, tile0 + ntiles) of the T * env_tiles tiles of the batch
  float clip_lo, clip_hi, beta, scale, inv_A;
  int mask_bytes;
  const void* actions;         // [T][E][N] masks / ids
  const float* logp_old;       // element (t, e, k) at t*st[0] + e*st[1] + k*st[2]
  const float* weight;
  int64_t lo_st[3], w_st[3];
  int tile0, ntiles, accumulate;
  float *g_w_ih, *g_w_hh, *g_b_ih, *g_b_hh, *g_w1, *g_b1, *g_w2, *g_b2, *stats;
  float *ws_x, *ws_h, *ws_g, *ws_y1, *ws_d1, *ws_dq, *ws_st;
};

// x image of the obs row (slot, env) of agent k: lane (g, i) <- x[sample i][16q + 4g + r]; zero: a front-padding
// step or a sample past E (nothing is read).  Record rows: one aligned dword per (q, lane) at byte 16q + 4g (inside
// the row: 16 IT <= RB), decoded as the MLP kernels do; columns >= F are forced to 0 -- byte F is those kernels'
// bias input 1, and the GRU here has its own biases -- so the image equals the fp32 path's on the decoded row.
template <bool REC>
__device__ __forceinline__ void load_x(const WideArgs& a, f32x4* xs, int k, int slot, int env, bool zero,
                                       const RecSigns<REC>& sg, int lane) {
  const int g = lane >> 4;
  const size_t r = ((size_t)slot * a.E + env) * a.N + k;
  if constexpr (REC) {
    const uint8_t* row = a.rec + r * a.RB;
    for (int q = 0; q < a.IT; ++q) {
      const int col = 16 * q + 4 * g;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (!zero) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(row + col);
        const uint32_t sm = sign_bytes(sg.bits4(col));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = col + e < a.F ? rec_byte(w, e, sm) : 0.f;
      }
      xs[q * 64 + lane] = v;
    }
    return;
  }
  const float* row = a.obs + r * a.F;
  for (int q = 0; q < a.IT; ++q) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!zero) v = wfrag(row, 1, a.F, 0, 16 * q + 4 * g, false);
    xs[q * 64 + lane] = v;
  }
}

// ------------------------------------------------------------------------------------------ policy / value
// One workgroup (one wave) per (tile, agent); a tile is 16 envs of one slot, so its window length is uniform.
// Unpadded windows run their S = min(p + 1, L) steps; front-zero-padded ones run all L, the zero-input steps being
// real steps (h moves through the biases, as preprocess_input_for_rnn's zeros do in the reference).  With carry_in
// the window is the carried h plus its last step -- the same step on the same h as the recompute's, hence bitwise.
template <int KIND, int MODE, bool REC>
__global__ __launch_bounds__(64) void gru_wide_policy_kernel(const WideArgs a) {
  __shared__ f32x4 xs[kMaxIT * 64], hb[2][kMaxHT * 64], qs[64];
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.y, tile = blockIdx.x;
  const int sl = tile / a.env_tiles, et = tile - sl * a.env_tiles;
  const int slot = a.slot0 + sl, env = 16 * et + i;
  const bool ok = env < a.E;
  const int envc = min(env, a.E - 1);
  const int pos = slot % a.ep_len, S = min(pos + 1, a.L), lo = slot - S + 1;
  const int pad = a.padded ? a.L - S : 0, steps = pad + S;
  const RecSigns<REC> sg(a, k);
  f32x4* hc = a.hcarry ? reinterpret_cast<f32x4*>(a.hcarry) + ((size_t)k * a.env_tiles + et) * a.HT * 64 : nullptr;
  const bool cin = hc && a.carry_in != 0;  // the host admits it for pos >= 1 only: the step below is never step 0
  for (int t = 0; t < a.HT; ++t) hb[0][t * 64 + lane] = cin ? hc[t * 64 + lane] : f32x4{0.f, 0.f, 0.f, 0.f};
  int cur = 0;
  for (int j = cin ? steps - 1 : 0; j < steps; ++j) {
    load_x<REC>(a, xs, k, lo + max(j - pad, 0), envc, j < pad || !ok, sg, lane);
    wave_sync();
    gru_step(a, k, xs, hb[cur], hb[cur ^ 1], j == 0, true, nullptr, lane);
    wave_sync();
    cur ^= 1;
  }
  if (hc && pos + 1 < a.L)  // the next slot's window extends this one
    for (int t = 0; t < a.HT; ++t) hc[t * 64 + lane] = hb[cur][t * 64 + lane];
  const int H = a.H;
  dense(a, a.w1 + (size_t)k * H * H, a.b1 + (size_t)k * H, H, a.HT, hb[cur], hb[cur ^ 1], true, lane);
  wave_sync();
  dense(a, a.w2 + (size_t)k * a.A * H, a.b2 + (size_t)k * a.A, a.A, 1, hb[cur ^ 1], qs, false, lane);
  f32x4 lg = qs[lane];  // outputs 4g + r of sample i (the lane's own store)
  const int samp = sl * a.E + env;  // slot-major sample index of the launch
  if constexpr (KIND == kWideValue) {
    if (ok && g == 0) a.value_out[(size_t)k * a.ep.E + samp] = lg[0];
  } else {
    const uint32_t rng = (MODE == kModeSample && a.ep.rng_off) ? a.ep.rng_step + *a.ep.rng_off : a.ep.rng_step;
#pragma unroll
    for (int r = 0; r < 4; ++r) lg[r] *= kLog2e;
    policy_epilogue<KIND == kWideBernoulli ? 0 : 1, false, false, MODE, false, KIND == kWideBernoulli>(
        a.ep, lg, 0.f, samp, ok, k, g, rng);
  }
}

// ------------------------------------------------------------------------------------------ PPO gradients
// forward + loss gradient + backward of one 16-sample tile of agent k (see the file comment)
template <int KIND, bool REC>
__global__ __launch_bounds__(64) void gru_wide_bptt_kernel(const WideArgs a) {
  __shared__ f32x4 xs[kMaxIT * 64], hb[3][kMaxHT * 64], dgs[3][kMaxHT * 64], qs[64];
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.y, tile = blockIdx.x, b = tile * 16 + i;
  const int HT = a.HT, HW = 16 * HT, IW = 16 * a.IT, L = a.L, H = a.H;
  const int Bp = 16 * a.ntiles;
  const int gt = a.tile0 + tile, slot = gt / a.env_tiles, et = gt - slot * a.env_tiles;
  const int env = 16 * et + i;
  const bool ok = env < a.E;
  const int envc = min(env, a.E - 1);
  const int pos = slot % a.ep_len, S = min(pos + 1, L), lo = slot - S + 1, pad = L - S;
  float* wx = a.ws_x + (size_t)k * L * Bp * IW;
  float* wh = a.ws_h + (size_t)k * (L + 1) * Bp * HW;
  float* wg = a.ws_g + (size_t)k * L * Bp * 4 * HW;
  const size_t hd = ((size_t)k * Bp + b) * HW;  // this sample's row of the head images

  for (int t = 0; t < HT; ++t) {
    hb[0][t * 64 + lane] = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(wh + (size_t)b * HW + 16 * t + 4 * g) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int cur = 0;
  const RecSigns<REC> sg(a, k);
  for (int j = 0; j < L; ++j) {
    load_x<REC>(a, xs, k, lo + max(j - pad, 0), envc, j < pad || !ok, sg, lane);
    for (int q = 0; q < a.IT; ++q)
      *reinterpret_cast<f32x4*>(wx + ((size_t)j * Bp + b) * IW + 16 * q + 4 * g) = xs[q * 64 + lane];
    wave_sync();
    gru_step(a, k, xs, hb[cur], hb[cur ^ 1], j == 0, true, wg + ((size_t)j * Bp + b) * 4 * HW, lane);
    cur ^= 1;
    for (int t = 0; t < HT; ++t)
      *reinterpret_cast<f32x4*>(wh + ((size_t)(j + 1) * Bp + b) * HW + 16 * t + 4 * g) = hb[cur][t * 64 + lane];
    wave_sync();
  }
  f32x4* y1 = hb[cur ^ 1];
  dense(a, a.w1 + (size_t)k * H * H, a.b1 + (size_t)k * H, H, HT, hb[cur], y1, true, lane);
  wave_sync();
  dense(a, a.w2 + (size_t)k * a.A * H, a.b2 + (size_t)k * a.A, a.A, 1, y1, qs, false, lane);
  const f32x4 lg = qs[lane];
  for (int t = 0; t < HT; ++t) *reinterpret_cast<f32x4*>(a.ws_y1 + hd + 16 * t + 4 * g) = y1[t * 64 + lane];

  // loss gradient w.r.t. the head outputs (ippo.py:178-217); samples past E contribute nothing
  const int64_t e64 = ok ? env : 0;
  const float W = a.weight[(int64_t)slot * a.w_st[0] + e64 * a.w_st[1] + (int64_t)k * a.w_st[2]];
  float st0 = 0.f, st1 = 0.f;
  f32x4 dlg;
  if constexpr (KIND == kWideValue) {
    const float d = lg[0] - W;  // V - R
    st0 = (ok && g == 0) ? d * d : 0.f;
    dlg = f32x4{(ok && g == 0) ? 2.f * a.scale * d : 0.f, 0.f, 0.f, 0.f};
  } else {
    const size_t cell = ((size_t)slot * a.E + (size_t)e64) * a.N + k;
    const uint32_t act = KIND == kWideCategorical ? reinterpret_cast<const unsigned char*>(a.actions)[cell]
                                                  : load_mask(a.actions, cell, a.mask_bytes);
    const float lp = a.logp_old[(int64_t)slot * a.lo_st[0] + e64 * a.lo_st[1] + (int64_t)k * a.lo_st[2]];
    dlg = ppo_dz<KIND == kWideBernoulli ? 0 : 1, false, KIND == kWideBernoulli>(a, lg, act, lp, W, ok, g, st0, st1);
  }
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) {  // lanes (0, i) hold the samples' terms
    st0 += __shfl_xor(st0, m);
    st1 += __shfl_xor(st1, m);
  }
  if (lane == 0) {
    a.ws_st[((size_t)k * a.ntiles + tile) * 2] = st0;
    a.ws_st[((size_t)k * a.ntiles + tile) * 2 + 1] = st1;
  }

  // backward through the head: dlg -> dpre1 -> dh_L
  *reinterpret_cast<f32x4*>(a.ws_dq + ((size_t)k * Bp + b) * 16 + 4 * g) = dlg;
  wave_sync();
  qs[lane] = dlg;
  wave_sync();
  f32x4* d1 = dgs[0];
  for (int t = 0; t < HT; ++t) {
    f32x4 acc = mat_t_vec(f32x4{0.f, 0.f, 0.f, 0.f}, a.w2 + (size_t)k * a.A * H, a.A, H, t, qs, 1, lane);
    const f32x4 y = y1[t * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = y[r] > 0.f ? acc[r] : 0.f;
    d1[t * 64 + lane] = acc;
    *reinterpret_cast<f32x4*>(a.ws_d1 + hd + 16 * t + 4 * g) = acc;
  }
  wave_sync();
  f32x4* dh = hb[2];
  f32x4* dhn = hb[cur];
  for (int t = 0; t < HT; ++t)
    dh[t * 64 + lane] = mat_t_vec(f32x4{0.f, 0.f, 0.f, 0.f}, a.w1 + (size_t)k * H * H, H, H, t, d1, HT, lane);
  wave_sync();

  // BPTT: the step's gates become its pre-activation gradients (dr, dz, dn_input, dn_recurrent) in place
  const float* Whh = a.w_hh + (size_t)k * 3 * H * H;
  for (int j = L - 1; j >= 0; --j) {
    float* gp = wg + ((size_t)j * Bp + b) * 4 * HW;
    const float* hp = wh + ((size_t)j * Bp + b) * HW;  // h before step j
    for (int t = 0; t < HT; ++t) {
      const int u0 = 16 * t + 4 * g;
      const f32x4 rv = *reinterpret_cast<const f32x4*>(gp + u0), zv = *reinterpret_cast<const f32x4*>(gp + HW + u0);
      const f32x4 nv = *reinterpret_cast<const f32x4*>(gp + 2 * HW + u0);
      const f32x4 nh = *reinterpret_cast<const f32x4*>(gp + 3 * HW + u0);
      const f32x4 ho = *reinterpret_cast<const f32x4*>(hp + u0);
      const f32x4 d = dh[t * 64 + lane];
      f32x4 dr, dz, dni, dnh, dd;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dn = d[r] * (1.f - zv[r]);
        dni[r] = dn * fmaf(-nv[r], nv[r], 1.f);
        dnh[r] = dni[r] * rv[r];
        dr[r] = dni[r] * nh[r] * (rv[r] * (1.f - rv[r]));
        dz[r] = d[r] * (ho[r] - nv[r]) * (zv[r] * (1.f - zv[r]));
        dd[r] = d[r] * zv[r];
      }
      *reinterpret_cast<f32x4*>(gp + u0) = dr;
      *reinterpret_cast<f32x4*>(gp + HW + u0) = dz;
      *reinterpret_cast<f32x4*>(gp + 2 * HW + u0) = dni;
      *reinterpret_cast<f32x4*>(gp + 3 * HW + u0) = dnh;
      dgs[0][t * 64 + lane] = dr;
      dgs[1][t * 64 + lane] = dz;
      dgs[2][t * 64 + lane] = dnh;
      dhn[t * 64 + lane] = dd;
    }
    if (j == 0) break;
    wave_sync();
    for (int t = 0; t < HT; ++t) {
      f32x4 acc = dhn[t * 64 + lane];
      acc = mat_t_vec(acc, Whh, H, H, t, dgs[0], HT, lane);
      acc = mat_t_vec(acc, Whh + (size_t)H * H, H, H, t, dgs[1], HT, lane);
      acc = mat_t_vec(acc, Whh + (size_t)2 * H * H, H, H, t, dgs[2], HT, lane);
      dh[t * 64 + lane] = acc;
    }
    wave_sync();
  }
}

// store_tile, added to what an earlier chunk left there (acc)
__device__ __forceinline__ void store_tile_acc(float* out, int rows, int cols, int r0, int c, f32x4 v, bool acc) {
  if (c >= cols) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r0 + r >= rows) continue;
    float* p = out + (size_t)(r0 + r) * cols + c;
    *p = acc ? *p + v[r] : v[r];
  }
}
__device__ __forceinline__ void store_acc(float* p, float v, bool acc) { *p = acc ? *p + v : v; }

__global__ __launch_bounds__(64) void gru_wide_wgrad_kernel(const WideArgs a) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.y, HT = a.HT, IT = a.IT, HW = 16 * HT, IW = 16 * IT, H = a.H, F = a.F, L = a.L;
  const int Bp = 16 * a.ntiles, KG = L * Bp;
  const bool acc = a.accumulate != 0;
  const float* wx = a.ws_x + (size_t)k * L * Bp * IW;
  const float* wh = a.ws_h + (size_t)k * (L + 1) * Bp * HW;
  const float* wg = a.ws_g + (size_t)k * L * Bp * 4 * HW;
  const float* hL = wh + (size_t)L * Bp * HW;
  const size_t hd = (size_t)k * Bp * HW;
  int j = blockIdx.x;
  if (j < 3 * HT * IT) {  // dW_ih
    const int G = j / (HT * IT), t = (j / IT) % HT, q = j % IT;
    const f32x4 v = outer_tile(wg + G * HW + 16 * t, 4 * HW, wx + 16 * q, IW, KG, lane);
    store_tile_acc(a.g_w_ih + ((size_t)k * 3 + G) * H * F, H, F, 16 * t + 4 * g, 16 * q + i, v, acc);
    return;
  }
  j -= 3 * HT * IT;
  if (j < 3 * HT * HT) {  // dW_hh (the n rows take the recurrent part's gradient)
    const int G = j / (HT * HT), t = (j / HT) % HT, q = j % HT;
    const f32x4 v = outer_tile(wg + (G < 2 ? G : 3) * HW + 16 * t, 4 * HW, wh + 16 * q, HW, KG, lane);
    store_tile_acc(a.g_w_hh + ((size_t)k * 3 + G) * H * H, H, H, 16 * t + 4 * g, 16 * q + i, v, acc);
    return;
  }
  j -= 3 * HT * HT;
  if (j < 4 * HT) {  // GRU biases
    const int G = j / HT, t = j % HT;
    const f32x4 v = outer_tile(wg + G * HW + 16 * t, 4 * HW, nullptr, 0, KG, lane);
    if (i == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int u = 16 * t + 4 * g + r;
        if (u >= H) continue;
        if (G != 3) store_acc(a.g_b_ih + (size_t)k * 3 * H + G * H + u, v[r], acc);
        if (G != 2) store_acc(a.g_b_hh + (size_t)k * 3 * H + (G == 3 ? 2 : G) * H + u, v[r], acc);
      }
    }
    return;
  }
  j -= 4 * HT;
  if (j < HT * HT) {  // dW1
    const int t = j / HT, q = j % HT;
    const f32x4 v = outer_tile(a.ws_d1 + hd + 16 * t, HW, hL + 16 * q, HW, Bp, lane);
    store_tile_acc(a.g_w1 + (size_t)k * H * H, H, H, 16 * t + 4 * g, 16 * q + i, v, acc);
    return;
  }
  j -= HT * HT;
  if (j < HT) {  // dW2
    const f32x4 v = outer_tile(a.ws_dq + (size_t)k * Bp * 16, 16, a.ws_y1 + hd + 16 * j, HW, Bp, lane);
    store_tile_acc(a.g_w2 + (size_t)k * a.A * H, a.A, H, 4 * g, 16 * j + i, v, acc);
    return;
  }
  j -= HT;
  if (j < HT) {  // db1
    const f32x4 v = outer_tile(a.ws_d1 + hd + 16 * j, HW, nullptr, 0, Bp, lane);
    if (i == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int u = 16 * j + 4 * g + r;
        if (u < H) store_acc(a.g_b1 + (size_t)k * H + u, v[r], acc);
      }
    }
    return;
  }
  // db2 and the loss sums
  const f32x4 v = outer_tile(a.ws_dq + (size_t)k * Bp * 16, 16, nullptr, 0, Bp, lane);
  if (i == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g + r < a.A) store_acc(a.g_b2 + (size_t)k * a.A + 4 * g + r, v[r], acc);
  }
  if (lane == 0 && a.stats) {
    float s0 = 0.f, s1 = 0.f;
    for (int t = 0; t < a.ntiles; ++t) {
      s0 += a.ws_st[((size_t)k * a.ntiles + t) * 2];
      s1 += a.ws_st[((size_t)k * a.ntiles + t) * 2 + 1];
    }
    store_acc(a.stats + (size_t)k * 2, s0, acc);
    store_acc(a.stats + (size_t)k * 2 + 1, s1, acc);
  }
}

int wgrad_tiles(int HT, int IT) { return 3 * HT * IT + 3 * HT * HT + 4 * HT + HT * HT + HT + HT + 1; }

// workspace floats of one (agent, tile): x, h (L + 1 states), the four gate rows, y1, dpre1, dlogits, two loss sums
int64_t tile_floats(int64_t L, int64_t HT, int64_t IT) {
  const int64_t HW = 16 * HT, IW = 16 * IT;
  return 16 * (L * IW + (L + 1) * HW + L * 4 * HW + 2 * HW + 16) + 2;
}

bool wide_shape(const d2d_gru_desc* d) {
  return d && d->hidden > kGruNarrowHidden && d->hidden <= kGruWideHidden && d->obs_dim >= 1 &&
         d->obs_dim + 1 <= 16 * kMaxIT && d->n_agents >= 0 && d->n_envs >= 0 && d->history_len >= 1;
}

int check_window(const d2d_gru_desc* d, const char* fn) {
  if (d->history_len > kMaxWindow) {
    d2d_set_error("%s: hidden > 64 supports history_len <= %d (got %d)", fn, kMaxWindow, d->history_len);
    return D2D_EUNSUPPORTED;
  }
  return D2D_OK;
}

WideArgs make_args(const d2d_gru_desc* d, int T, const void* obs) {
  WideArgs a = {};
  a.N = d->n_agents; a.E = d->n_envs; a.F = d->obs_dim; a.H = d->hidden;
  a.A = d->kind == 2 ? 1 : d->n_out; a.kind = d->kind;
  a.HT = (a.H + 15) / 16; a.IT = (a.F + 15) / 16;
  a.T = T; a.L = d->history_len; a.ep_len = d->episode_length; a.env_tiles = (a.E + 15) / 16;
  a.vecF = a.F % 4 == 0 && aligned16(d->w_ih);
  a.vecH = a.H % 4 == 0 && aligned16(d->w_hh) && aligned16(d->w1) && aligned16(d->w2);
  a.w_ih = d->w_ih; a.w_hh = d->w_hh; a.b_ih = d->b_ih; a.b_hh = d->b_hh;
  a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2; a.b2 = d->b2;
  obs_format_args(d->obs_format, d->obs_signed, d->obs_dim, obs, a.obs, a.rec, a.sgn);  // checked by the caller
  a.RB = D2D_RECORD_BYTES(a.F);
  a.inv_A = 1.f / (float)a.A;
  a.mask_bytes = a.A <= 8 ? 1 : a.A <= 16 ? 2 : 4;
  return a;
}

template <int KIND, bool REC>
void launch_policy(const WideArgs& a, dim3 grid, hipStream_t s) {
  if (KIND == kWideValue || a.ep.forced == nullptr) {
    if (KIND != kWideValue && a.ep.deterministic)
      hipLaunchKernelGGL((gru_wide_policy_kernel<KIND, kModeDeterministic, REC>), grid, dim3(64), 0, s, a);
    else
      hipLaunchKernelGGL((gru_wide_policy_kernel<KIND, kModeSample, REC>), grid, dim3(64), 0, s, a);
  } else {
    hipLaunchKernelGGL((gru_wide_policy_kernel<KIND, kModeForced, REC>), grid, dim3(64), 0, s, a);
  }
}
template <bool REC>
void launch_policy_kind(const WideArgs& a, dim3 grid, hipStream_t s) {
  if (a.kind == kWideBernoulli) launch_policy<kWideBernoulli, REC>(a, grid, s);
  else if (a.kind == kWideCategorical) launch_policy<kWideCategorical, REC>(a, grid, s);
  else launch_policy<kWideValue, REC>(a, grid, s);
}
template <bool REC>
void launch_bptt(const WideArgs& a, dim3 grid, hipStream_t s) {
  if (a.kind == kWideBernoulli) hipLaunchKernelGGL((gru_wide_bptt_kernel<kWideBernoulli, REC>), grid, dim3(64), 0, s, a);
  else if (a.kind == kWideCategorical)
    hipLaunchKernelGGL((gru_wide_bptt_kernel<kWideCategorical, REC>), grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL((gru_wide_bptt_kernel<kWideValue, REC>), grid, dim3(64), 0, s, a);
}

}  // namespace

int64_t gru_wide_carry_floats(const d2d_gru_desc* d) {
  if (!wide_shape(d)) return -1;
  return (int64_t)d->n_agents * (16 * (((int64_t)d->n_envs + 15) / 16)) * (16 * ((d->hidden + 15) / 16));
}

// the entry points of gru_kernels.hip have checked the desc (check_gru_desc), the buffers and the slot range
int gru_wide_policy(const d2d_gru_desc* d, int32_t T, const void* obs, int32_t slot0, int32_t n_slots, int32_t padded,
                    const void* forced, uint32_t rng_step, int32_t deterministic, void* actions, float* out,
                    float* hcarry, int32_t carry_in, void* stream) {
  int rc = check_window(d, "d2d_policy_gru");
  if (rc) return rc;
  if (hcarry && !aligned16(hcarry)) { d2d_set_error("d2d_policy_gru_carry: hcarry must be 16-byte aligned"); return D2D_EINVAL; }
  WideArgs a = make_args(d, T, obs);
  a.slot0 = slot0; a.n_slots = n_slots; a.padded = padded ? 1 : 0;
  a.hcarry = hcarry; a.carry_in = carry_in ? 1 : 0;
  MlpArgs& ep = a.ep;
  ep.E = n_slots * a.E; ep.N = a.N; ep.F = a.F; ep.H = a.H; ep.A = a.A; ep.kind = d->kind == 0 ? 0 : 1;
  ep.deterministic = deterministic ? 1 : 0; ep.inv_A = a.inv_A; ep.rng_step = rng_step; ep.rng_off = d->rng_offset;
  ep.seed = d->seed; ep.env_base = d->env_base; ep.forced = forced; ep.act_out = actions; ep.logp_out = out;
  ep.value_out = nullptr; ep.mask_bytes = a.mask_bytes;
  a.value_out = out;
  if (a.N == 0 || a.E == 0 || n_slots == 0) return D2D_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)((int64_t)n_slots * a.env_tiles), a.N);
  if (a.rec) launch_policy_kind<true>(a, grid, s);
  else launch_policy_kind<false>(a, grid, s);
  D2D_CHECK_HIP(hipGetLastError());
  return D2D_OK;
}

int64_t gru_wide_grad_workspace(const d2d_gru_desc* d, int32_t T) {
  if (!wide_shape(d) || d->n_agents <= 0 || T <= 0 || d->n_envs <= 0 || d->history_len > kMaxWindow) return 0;
  const int64_t per = (int64_t)d->n_agents * tile_floats(d->history_len, (d->hidden + 15) / 16, (d->obs_dim + 15) / 16);
  const int64_t tiles = (int64_t)T * ((d->n_envs + 15) / 16);
  return per * std::max<int64_t>(1, std::min<int64_t>(tiles, kGruWideBudgetFloats / per));
}

int gru_wide_grad(const d2d_gru_desc* d, int32_t T, const void* obs, const void* actions, const float* logp_old,
                  const int64_t* logp_strides, const float* weight, const int64_t* weight_strides, float clip,
                  float beta, float scale, float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_w1,
                  float* g_b1, float* g_w2, float* g_b2, float* stats, float* workspace, int64_t workspace_floats,
                  void* stream) {
  int rc = check_window(d, "d2d_gru_grad");
  if (rc) return rc;
  WideArgs a = make_args(d, T, obs);
  a.actions = actions; a.logp_old = logp_old; a.weight = weight;
  for (int q = 0; q < 3; ++q) {
    a.lo_st[q] = logp_strides ? logp_strides[q] : 0;
    a.w_st[q] = weight_strides[q];
  }
  a.clip_lo = 1.f - clip; a.clip_hi = 1.f + clip; a.beta = beta; a.scale = scale;
  a.g_w_ih = g_w_ih; a.g_w_hh = g_w_hh; a.g_b_ih = g_b_ih; a.g_b_hh = g_b_hh;
  a.g_w1 = g_w1; a.g_b1 = g_b1; a.g_w2 = g_w2; a.g_b2 = g_b2; a.stats = stats;
  if (a.N == 0) return D2D_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t tiles = (int64_t)T * a.env_tiles;
  if (tiles == 0) {
    // an empty batch (T = 0 or no envs): every gradient and loss sum is zero, and nothing touches `workspace`
    const size_t H = (size_t)a.H, N = (size_t)a.N, F = (size_t)a.F, A = (size_t)a.A, f = sizeof(float);
    D2D_CHECK_HIP(hipMemsetAsync(g_w_ih, 0, f * N * 3 * H * F, s));
    D2D_CHECK_HIP(hipMemsetAsync(g_w_hh, 0, f * N * 3 * H * H, s));
    D2D_CHECK_HIP(hipMemsetAsync(g_b_ih, 0, f * N * 3 * H, s));
    D2D_CHECK_HIP(hipMemsetAsync(g_b_hh, 0, f * N * 3 * H, s));
    D2D_CHECK_HIP(hipMemsetAsync(g_w1, 0, f * N * H * H, s));
    D2D_CHECK_HIP(hipMemsetAsync(g_b1, 0, f * N * H, s));
    D2D_CHECK_HIP(hipMemsetAsync(g_w2, 0, f * N * A * H, s));
    D2D_CHECK_HIP(hipMemsetAsync(g_b2, 0, f * N * A, s));
    if (stats) {
      D2D_CHECK_HIP(hipMemsetAsync(stats, 0, f * N * 2, s));
    }
    return D2D_OK;
  }
  // chunks of whole tiles: as many tiles of every agent as the workspace holds
  const int64_t HW = 16 * a.HT, IW = 16 * a.IT, L = a.L, N = a.N;
  const int64_t per = N * tile_floats(L, a.HT, a.IT);
  // (a chunk's step x sample count stays an int)
  const int64_t C = std::min<int64_t>({tiles, workspace_floats / per, ((int64_t)1 << 30) / (16 * L)});
  if (C < 1 || !aligned16(workspace)) {
    d2d_set_error("d2d_gru_grad: workspace of %lld floats, one tile of every agent takes %lld (16-byte aligned; "
                  "d2d_gru_grad_workspace asks for %lld)", (long long)workspace_floats, (long long)per,
                  (long long)gru_wide_grad_workspace(d, T));
    return D2D_EINVAL;
  }
  const int64_t Cp = 16 * C;
  int64_t o = 0;
  a.ws_x = workspace + o; o += N * L * Cp * IW;
  a.ws_h = workspace + o; o += N * (L + 1) * Cp * HW;
  a.ws_g = workspace + o; o += N * L * Cp * 4 * HW;
  a.ws_y1 = workspace + o; o += N * Cp * HW;
  a.ws_d1 = workspace + o; o += N * Cp * HW;
  a.ws_dq = workspace + o; o += N * Cp * 16;
  a.ws_st = workspace + o;
  for (int64_t t0 = 0; t0 < tiles; t0 += C) {
    a.tile0 = (int)t0; a.ntiles = (int)std::min<int64_t>(C, tiles - t0); a.accumulate = t0 > 0;
    const dim3 grid((unsigned)a.ntiles, a.N);
    if (a.rec) launch_bptt<true>(a, grid, s);
    else launch_bptt<false>(a, grid, s);
    D2D_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(gru_wide_wgrad_kernel, dim3(wgrad_tiles(a.HT, a.IT), a.N), dim3(64), 0, s, a);
    D2D_CHECK_HIP(hipGetLastError());
  }
  return D2D_OK;
}

}  // namespace d2d
