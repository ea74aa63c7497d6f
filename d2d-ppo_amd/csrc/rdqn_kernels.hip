// iRDQN (the reference's value-based baseline, /root/reference/algorithms/irdqn.py:58-86, 133-148, 154) on
// gfx950: Q-values / epsilon-greedy actions of observation windows (d2d_rdqn_q) and one TD update's gradients
// (d2d_rdqn_grad) for every agent in one call.
//
//   network: GRU(F, H) -> Linear(H, H) -> ReLU -> Linear(H, H) -> ReLU -> Linear(H, A), h0 = 0 per window,
//   torch's GRU formula and gate order (gru_common.h:5-8).
//
// Layout (v_mfma_f32_16x16x4_f32, lane = (g, i), g = lane >> 4, i = lane & 15, as gru_common.h): one 16-sample
// tile per wave and one wave per workgroup, the sample on i; every layer is computed transposed,
// Y^T[row][sample] = W . V^T, so an accumulator tile holds rows 16t + 4g + r of sample i -- exactly the B operand
// of the next product with the k order permuted (k-step r of k-tile q <-> column 16q + 4g + r).  Every product is
// exact in fp32, accumulated in fp32.
//
// H goes up to 128 here (the learner's default is 100), so the register-resident vectors of gru_kernels.hip
// (H <= 64, tile counts as template parameters) do not fit, and an fp32 W_hh image padded to 112 / 128 columns
// does not fit the LDS next to W_ih.  Instead
//   - the hidden tile count HT = ceil(H / 16) is a run-time value: vectors (x, h, the head activations, dh and the
//     gate gradients) live in LDS as "vector images" V[tile][lane] of f32x4 in accumulator layout (8 KB each at
//     HT = 8), read back by the same lane as B operands (no bank conflicts: consecutive lanes, 16 bytes each);
//   - weight fragments come straight from the agent-stacked torch tensors in global memory (~240 KB per agent
//     at H = 100: L2-resident, shared by all tiles of an agent), as one 16-byte load per fragment where the row
//     length is a multiple of 4 and as masked scalar loads otherwise.  Rows / columns past H, F or A read as exact
//     zeros, so padded hidden units stay exactly 0 and never reach an output.
//
// The helpers of this layout that do not depend on the Q head or the replay ring (wfrag, bfrag, mat_vec, mat_t_vec,
// RecSigns, gru_step, dense, outer_tile, store_tile) live in gru_l2_common.h, which the wide PPO GRU kernels
// (gru_wide_kernels.hip) share.
//
// d2d_rdqn_grad runs two kernels.  (1) rdqn_bptt_kernel, per (agent, tile): forward over the L steps keeping x, h
// and the gates (r, z, n, W_hn h + b_hn) in the caller's workspace, head forward, TD loss, backward through the head
// and BPTT, which overwrites each step's gates with its pre-activation gradients.  (2) rdqn_wgrad_kernel, one wave
// per 16 x 16 tile of a gradient tensor: dW = sum over (step, sample) of dpre (x) input as MFMA products over the
// workspace images, in a fixed order with no atomics -- bitwise reproducible.
//
// Observations enter through load_x alone: fp32 ring rows, or (d2d_rdqn_q_ex / d2d_rdqn_grad_ex, D2D_OBS_U8) the env
// kernel's compact record decoded to the same floats.  d2d_rdqn_q_ex can also keep every sample's final h in a
// scratch (hcarry) and start the next acting slot from it -- one GRU step instead of the window, the same arithmetic.
#include <algorithm>
#include <string>

#include "common.h"
#include "gru_common.h"
#include "gru_l2_common.h"

namespace d2d {
namespace {

constexpr uint32_t kStreamRdqn = 4;  // Philox stream of the epsilon-greedy draw (3 = policy sampling)

struct RdqnArgs {
  int N, E, F, H, A, HT, IT;
  int vecF, vecH;              // 16-byte fragment loads of F-wide / H-wide rows
  const float *w_ih, *w_hh, *b_ih, *b_hh, *w1, *b1, *w2, *b2, *w3, *b3;
  const float* obs;            // ring [rows][E][N][F] (fp32 rows; else rec below)
  int rows, ep_len, shift;     // ep_len > 0: window indices are transitions, row = m + m / ep_len + shift
  int ntrans;                  // ep_len > 0: transitions the ring holds per env
  const int32_t* samples;      // [B][3] env, last, window length
  int B, mask_bytes;
  // q kernel
  int mode, ready;
  float eps;
  const float* eps_rows;       // optional per-sample epsilon (overrides eps)
  const uint8_t *explore_mask, *explore_action;
  uint32_t rng_step;
  const uint32_t* rng_off;
  uint64_t seed, env_base;
  float *q, *qmax;
  void* action;
  // grad kernels
  int L, ntiles, huber;
  float gamma;
  const void* act_in;
  const float *reward, *qmax_target;
  const uint8_t* done;
  float *g_w_ih, *g_w_hh, *g_b_ih, *g_b_hh, *g_w1, *g_b1, *g_w2, *g_b2, *g_w3, *g_b3, *loss;
  float *ws_x, *ws_h, *ws_g, *ws_y1, *ws_y2, *ws_d1, *ws_d2, *ws_dq, *ws_loss;
  // the kernels' REC / CARRY instances only (after the fields every instance reads, which keep their offsets)
  const uint8_t* rec;          // the compact record [rows][E][N][RB] (D2D_OBS_U8) in place of obs, with
  const uint32_t* sgn;         // its int8-column masks [N][RB / 32]
  int RB;
  int carry_in;                // h0 = hcarry and one step on row `last` instead of the whole window
  float* hcarry;               // [N][tiles][HT][64] f32x4: the final h image of every (agent, tile)
};

// ring row of window index m (any sign) of this launch
__device__ __forceinline__ int ring_row(const RdqnArgs& a, int m) {
  if (a.ep_len > 0) {
    m %= a.ntrans;
    if (m < 0) m += a.ntrans;
    int row = m + m / a.ep_len + a.shift;
    return row % a.rows;
  }
  m %= a.rows;
  return m < 0 ? m + a.rows : m;
}

// x image of one window step: lane (g, i) <- x[sample i][16q + 4g + r]; zero: the window has not started.
// Record rows: one aligned dword per (q, lane) at byte 16q + 4g (inside the row: 16 IT <= RB), decoded as the MLP
// kernels do; columns >= F are forced to 0 -- byte F is those kernels' bias input 1, and the GRU here has its own
// biases -- so the image, and ws_x after it, equal the fp32 path's on the decoded row.
template <bool REC>
__device__ __forceinline__ void load_x(const RdqnArgs& a, f32x4* xs, int k, int env, int m, bool zero,
                                       const RecSigns<REC>& sg, int lane) {
  const int g = lane >> 4;
  if constexpr (REC) {
    const size_t r = ((size_t)ring_row(a, m) * a.E + env) * a.N + k;
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
  const float* row = a.obs + (((size_t)ring_row(a, m) * a.E + env) * a.N + k) * a.F;
  for (int q = 0; q < a.IT; ++q) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!zero) v = wfrag(row, 1, a.F, 0, 16 * q + 4 * g, false);
    xs[q * 64 + lane] = v;
  }
}

// the three head layers on the image h (buffers y1, y2 as scratch): returns Q[4g + r] of sample i
__device__ __forceinline__ f32x4 head_fwd(const RdqnArgs& a, int k, const f32x4* h, f32x4* y1, f32x4* y2, f32x4* qs,
                                          int lane) {
  const int H = a.H;
  dense(a, a.w1 + (size_t)k * H * H, a.b1 + (size_t)k * H, H, a.HT, h, y1, true, lane);
  wave_sync();
  dense(a, a.w2 + (size_t)k * H * H, a.b2 + (size_t)k * H, H, a.HT, y1, y2, true, lane);
  wave_sync();
  dense(a, a.w3 + (size_t)k * a.A * H, a.b3 + (size_t)k * a.A, a.A, 1, y2, qs, false, lane);
  return qs[lane];
}

struct Best {
  float v;
  int idx;
};
__device__ __forceinline__ Best better(Best x, Best y) {  // the larger value, the lower index on ties
  return (y.v > x.v || (y.v == x.v && y.idx < x.idx)) ? y : x;
}

// max and lowest-index argmax over the A actions of sample i (in every lane of the sample)
__device__ __forceinline__ Best q_best(f32x4 q, int A, int lane) {
  const int g = lane >> 4;
  Best b = {-INFINITY, 4 * g};
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (4 * g + r < A) b = better(b, Best{q[r], 4 * g + r});
#pragma unroll
  for (int m = 16; m <= 32; m <<= 1) {
    Best o = {__shfl_xor(b.v, m), __shfl_xor(b.idx, m)};
    b = better(b, o);
  }
  return b;
}

// ------------------------------------------------------------------------------------------ Q / acting
// REC: observations from the compact record.  CARRY: hcarry is given -- the final h is stored there, and with
// carry_in the window is the carried h plus one step.  <false, false> is the kernel of d2d_rdqn_q as it always was.
template <bool REC, bool CARRY>
__global__ __launch_bounds__(64) void rdqn_q_kernel(const RdqnArgs a) {
  __shared__ f32x4 xs[kMaxIT * 64], hb[3][kMaxHT * 64], qs[64];
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.y, b = blockIdx.x * 16 + i;
  const bool ok = b < a.B;
  const int bs = ok ? b : a.B - 1;
  int env = a.samples[3 * bs], last = a.samples[3 * bs + 1], S = a.samples[3 * bs + 2];
  env = min(max(env, 0), a.E - 1);
  S = min(max(S, 1), kMaxWindow);
  int Smax = S;
#pragma unroll
  for (int m = 1; m <= 8; m <<= 1) Smax = max(Smax, __shfl_xor(Smax, m));
  Smax = __builtin_amdgcn_readfirstlane(Smax);
  const RecSigns<REC> sg(a, k);
  // carried state: this (agent, tile)'s h image as the previous launch left it (the contract of d2d_rdqn_q_ex)
  const bool cin = CARRY && a.carry_in != 0;
  f32x4* hc = nullptr;
  if constexpr (CARRY) hc = reinterpret_cast<f32x4*>(a.hcarry) + ((size_t)k * gridDim.x + blockIdx.x) * a.HT * 64;
  for (int t = 0; t < a.HT; ++t) hb[0][t * 64 + lane] = cin ? hc[t * 64 + lane] : f32x4{0.f, 0.f, 0.f, 0.f};
  int cur = 0;
  const int steps = cin ? 1 : Smax;  // carry-in: the one new row of every sample, on the carried h
  for (int j = 0; j < steps; ++j) {
    const int rel = cin ? S - 1 : j - (Smax - S);  // step of this sample's own window (right-aligned)
    const bool active = rel >= 0;
    load_x<REC>(a, xs, k, env, last - S + 1 + max(rel, 0), !active, sg, lane);
    wave_sync();
    gru_step(a, k, xs, hb[cur], hb[cur ^ 1], !cin && j == 0, active, nullptr, lane);
    wave_sync();
    cur ^= 1;
  }
  if constexpr (CARRY)
    for (int t = 0; t < a.HT; ++t) hc[t * 64 + lane] = hb[cur][t * 64 + lane];
  const f32x4 q = head_fwd(a, k, hb[cur], hb[cur ^ 1], hb[2], qs, lane);
  if (ok && a.q) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g + r < a.A) a.q[((size_t)k * a.B + b) * a.A + 4 * g + r] = q[r];
  }
  const Best best = q_best(q, a.A, lane);
  if (!ok || g != 0) return;
  if (a.qmax) a.qmax[(size_t)k * a.B + b] = best.v;
  if (!a.action) return;
  int act = best.idx;
  const size_t o = (size_t)b * a.N + k;
  if (a.mode == 1) {
    const uint32_t rng = a.rng_step + (a.rng_off ? *a.rng_off : 0u);
    const u32x4 w = philox((uint32_t)(a.env_base + (uint64_t)env), (uint32_t)k, rng, kStreamRdqn << 24, a.seed);
    const float u = (float)(w.x >> 8) * 5.9604644775390625e-08f;  // [0, 1) on 24 bits
    const float eps = a.eps_rows ? a.eps_rows[b] : a.eps;
    if (!(a.ready && u >= eps)) act = (int)(w.y & 1u);          // irdqn.py:154: np.random.randint(0, 2)
  } else if (a.mode == 2) {
    if (a.explore_mask[o]) act = a.explore_action[o];
  }
  const uint32_t mask = 1u << act;
  if (a.mask_bytes == 1) static_cast<uint8_t*>(a.action)[o] = (uint8_t)mask;
  else static_cast<uint16_t*>(a.action)[o] = (uint16_t)mask;
}

// ------------------------------------------------------------------------------------------ TD gradients
// forward + loss + backward of one 16-sample tile of agent k (see the file comment)
template <bool REC>
__global__ __launch_bounds__(64) void rdqn_bptt_kernel(const RdqnArgs a) {
  __shared__ f32x4 xs[kMaxIT * 64], hb[3][kMaxHT * 64], dgs[3][kMaxHT * 64], qs[64];
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.y, tile = blockIdx.x, b = tile * 16 + i;
  const int HT = a.HT, HW = 16 * HT, IW = 16 * a.IT, L = a.L, H = a.H;
  const int Bp = 16 * a.ntiles;
  const bool ok = b < a.B;
  const int bs = ok ? b : a.B - 1;
  const int env = min(max(a.samples[3 * bs], 0), a.E - 1), last = a.samples[3 * bs + 1];
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
    load_x<REC>(a, xs, k, env, last - L + 1 + j, false, sg, lane);
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
  f32x4* y2 = hb[2];
  const f32x4 q = head_fwd(a, k, hb[cur], y1, y2, qs, lane);
  for (int t = 0; t < HT; ++t) {
    *reinterpret_cast<f32x4*>(a.ws_y1 + hd + 16 * t + 4 * g) = y1[t * 64 + lane];
    *reinterpret_cast<f32x4*>(a.ws_y2 + hd + 16 * t + 4 * g) = y2[t * 64 + lane];
  }

  // TD loss of the window's last transition (irdqn.py:133-148, 292-297)
  const size_t o = (size_t)bs * a.N + k;
  const uint32_t am = a.mask_bytes == 1 ? static_cast<const uint8_t*>(a.act_in)[o]
                                        : static_cast<const uint16_t*>(a.act_in)[o];
  const int act = am ? __builtin_ctz(am) : -1;
  float qa = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (4 * g + r == act) qa = q[r];
  qa += __shfl_xor(qa, 16);
  qa += __shfl_xor(qa, 32);
  const float nd = a.done[bs] ? 0.f : 1.f;
  const float td = fmaf(nd * a.gamma, a.qmax_target[(size_t)k * a.B + bs], a.reward[o]);
  const float delta = qa - td, ad = fabsf(delta), invB = 1.f / (float)a.B;
  float ls, coef;
  if (a.huber) {
    ls = ad < 1.f ? 0.5f * delta * delta : ad - 0.5f;
    coef = fminf(fmaxf(delta, -1.f), 1.f) * invB;
  } else {
    ls = delta * delta;
    coef = 2.f * delta * invB;
  }
  if (!ok || act < 0 || act >= a.A) { ls = 0.f; coef = 0.f; }
  if (g != 0) ls = 0.f;
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) ls += __shfl_xor(ls, m);
  if (lane == 0) a.ws_loss[(size_t)k * a.ntiles + tile] = ls;

  // backward through the head: dq -> dpre2 -> dpre1 -> dh_L
  f32x4 dq;
#pragma unroll
  for (int r = 0; r < 4; ++r) dq[r] = (4 * g + r == act) ? coef : 0.f;
  *reinterpret_cast<f32x4*>(a.ws_dq + ((size_t)k * Bp + b) * 16 + 4 * g) = dq;
  wave_sync();
  qs[lane] = dq;
  wave_sync();
  f32x4* d2 = dgs[0];
  f32x4* d1 = dgs[1];
  for (int t = 0; t < HT; ++t) {
    f32x4 acc = mat_t_vec(f32x4{0.f, 0.f, 0.f, 0.f}, a.w3 + (size_t)k * a.A * H, a.A, H, t, qs, 1, lane);
    const f32x4 y = y2[t * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = y[r] > 0.f ? acc[r] : 0.f;
    d2[t * 64 + lane] = acc;
    *reinterpret_cast<f32x4*>(a.ws_d2 + hd + 16 * t + 4 * g) = acc;
  }
  wave_sync();
  for (int t = 0; t < HT; ++t) {
    f32x4 acc = mat_t_vec(f32x4{0.f, 0.f, 0.f, 0.f}, a.w2 + (size_t)k * H * H, H, H, t, d2, HT, lane);
    const f32x4 y = y1[t * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = y[r] > 0.f ? acc[r] : 0.f;
    d1[t * 64 + lane] = acc;
    *reinterpret_cast<f32x4*>(a.ws_d1 + hd + 16 * t + 4 * g) = acc;
  }
  wave_sync();
  f32x4* dh = hb[0];
  f32x4* dhn = hb[1];
  for (int t = 0; t < HT; ++t)
    dh[t * 64 + lane] = mat_t_vec(f32x4{0.f, 0.f, 0.f, 0.f}, a.w1 + (size_t)k * H * H, H, H, t, d1, HT, lane);
  wave_sync();

  // BPTT: the step's gates become its pre-activation gradients (dr, dz, dn_input, dn_recurrent) in place
  const float* Whh = a.w_hh + (size_t)k * 3 * H * H;
  for (int j = L - 1; j >= 0; --j) {
    float* gt = wg + ((size_t)j * Bp + b) * 4 * HW;
    const float* hp = wh + ((size_t)j * Bp + b) * HW;  // h before step j
    for (int t = 0; t < HT; ++t) {
      const int u0 = 16 * t + 4 * g;
      const f32x4 rv = *reinterpret_cast<const f32x4*>(gt + u0), zv = *reinterpret_cast<const f32x4*>(gt + HW + u0);
      const f32x4 nv = *reinterpret_cast<const f32x4*>(gt + 2 * HW + u0);
      const f32x4 nh = *reinterpret_cast<const f32x4*>(gt + 3 * HW + u0);
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
      *reinterpret_cast<f32x4*>(gt + u0) = dr;
      *reinterpret_cast<f32x4*>(gt + HW + u0) = dz;
      *reinterpret_cast<f32x4*>(gt + 2 * HW + u0) = dni;
      *reinterpret_cast<f32x4*>(gt + 3 * HW + u0) = dnh;
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

__global__ __launch_bounds__(64) void rdqn_wgrad_kernel(const RdqnArgs a) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int k = blockIdx.y, HT = a.HT, IT = a.IT, HW = 16 * HT, IW = 16 * IT, H = a.H, F = a.F, L = a.L;
  const int Bp = 16 * a.ntiles, KG = L * Bp;
  const float* wx = a.ws_x + (size_t)k * L * Bp * IW;
  const float* wh = a.ws_h + (size_t)k * (L + 1) * Bp * HW;
  const float* wg = a.ws_g + (size_t)k * L * Bp * 4 * HW;
  const float* hL = wh + (size_t)L * Bp * HW;
  const size_t hd = (size_t)k * Bp * HW;
  int j = blockIdx.x;
  if (j < 3 * HT * IT) {  // dW_ih
    const int G = j / (HT * IT), t = (j / IT) % HT, q = j % IT;
    const f32x4 v = outer_tile(wg + G * HW + 16 * t, 4 * HW, wx + 16 * q, IW, KG, lane);
    store_tile(a.g_w_ih + ((size_t)k * 3 + G) * H * F, H, F, 16 * t + 4 * g, 16 * q + i, v);
    return;
  }
  j -= 3 * HT * IT;
  if (j < 3 * HT * HT) {  // dW_hh (the n rows take the recurrent part's gradient)
    const int G = j / (HT * HT), t = (j / HT) % HT, q = j % HT;
    const f32x4 v = outer_tile(wg + (G < 2 ? G : 3) * HW + 16 * t, 4 * HW, wh + 16 * q, HW, KG, lane);
    store_tile(a.g_w_hh + ((size_t)k * 3 + G) * H * H, H, H, 16 * t + 4 * g, 16 * q + i, v);
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
        if (G != 3) a.g_b_ih[(size_t)k * 3 * H + G * H + u] = v[r];
        if (G != 2) a.g_b_hh[(size_t)k * 3 * H + (G == 3 ? 2 : G) * H + u] = v[r];
      }
    }
    return;
  }
  j -= 4 * HT;
  if (j < 2 * HT * HT) {  // dW1, dW2
    const int second = j >= HT * HT, jj = j - second * HT * HT, t = jj / HT, q = jj % HT;
    const float* A = (second ? a.ws_d2 : a.ws_d1) + hd + 16 * t;
    const float* Bm = second ? a.ws_y1 + hd + 16 * q : hL + 16 * q;
    const f32x4 v = outer_tile(A, HW, Bm, HW, Bp, lane);
    store_tile((second ? a.g_w2 : a.g_w1) + (size_t)k * H * H, H, H, 16 * t + 4 * g, 16 * q + i, v);
    return;
  }
  j -= 2 * HT * HT;
  if (j < HT) {  // dW3
    const f32x4 v = outer_tile(a.ws_dq + (size_t)k * Bp * 16, 16, a.ws_y2 + hd + 16 * j, HW, Bp, lane);
    store_tile(a.g_w3 + (size_t)k * a.A * H, a.A, H, 4 * g, 16 * j + i, v);
    return;
  }
  j -= HT;
  if (j < 2 * HT) {  // db1, db2
    const int second = j >= HT, t = j - second * HT;
    const f32x4 v = outer_tile((second ? a.ws_d2 : a.ws_d1) + hd + 16 * t, HW, nullptr, 0, Bp, lane);
    if (i == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int u = 16 * t + 4 * g + r;
        if (u < H) (second ? a.g_b2 : a.g_b1)[(size_t)k * H + u] = v[r];
      }
    }
    return;
  }
  // db3 and the loss
  const f32x4 v = outer_tile(a.ws_dq + (size_t)k * Bp * 16, 16, nullptr, 0, Bp, lane);
  if (i == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g + r < a.A) a.g_b3[(size_t)k * a.A + 4 * g + r] = v[r];
  }
  if (lane == 0) {
    float s = 0.f;
    for (int t = 0; t < a.ntiles; ++t) s += a.ws_loss[(size_t)k * a.ntiles + t];
    a.loss[k] = s / (float)a.B;
  }
}

int wgrad_tiles(int HT, int IT) { return 3 * HT * IT + 3 * HT * HT + 4 * HT + 2 * HT * HT + HT + 2 * HT + 1; }

// float offsets of the workspace pieces; returns the total
struct WsLayout {
  int64_t x, h, g, y1, y2, d1, d2, dq, loss, total;
};
WsLayout ws_layout(int64_t N, int64_t L, int64_t B, int64_t HT, int64_t IT) {
  const int64_t nt = (B + 15) / 16, Bp = 16 * nt, HW = 16 * HT, IW = 16 * IT;
  WsLayout w;
  int64_t o = 0;
  w.x = o; o += N * L * Bp * IW;
  w.h = o; o += N * (L + 1) * Bp * HW;
  w.g = o; o += N * L * Bp * 4 * HW;
  w.y1 = o; o += N * Bp * HW;
  w.y2 = o; o += N * Bp * HW;
  w.d1 = o; o += N * Bp * HW;
  w.d2 = o; o += N * Bp * HW;
  w.dq = o; o += N * Bp * 16;
  w.loss = o; o += N * nt;
  w.total = o;
  return w;
}

int check_desc(const d2d_rdqn_desc* d, const char* fn) {
  if (!d) { d2d_set_error("%s: NULL desc", fn); return D2D_EINVAL; }
  if (d->n_agents < 0 || d->n_envs < 1 || d->obs_dim < 1 || d->hidden < 1 || d->n_out < 1 || d->ring_rows < 1 ||
      d->ring_episode < 0) {
    d2d_set_error("%s: bad shape", fn);
    return D2D_EINVAL;
  }
  if (d->hidden > 16 * kMaxHT || d->obs_dim + 1 > 16 * kMaxIT || d->n_out > 16) {
    d2d_set_error("%s: supports hidden <= 128, obs_dim + 1 <= 64, n_out <= 16 (got hidden %d, obs_dim %d, n_out %d)",
                  fn, d->hidden, d->obs_dim, d->n_out);
    return D2D_EUNSUPPORTED;
  }
  if (d->ring_episode > 0 && d->ring_rows % (d->ring_episode + 1) != 0) {
    d2d_set_error("%s: ring_rows %d is not whole episodes of %d + 1 rows", fn, d->ring_rows, d->ring_episode);
    return D2D_EINVAL;
  }
  if (!d->w_ih || !d->w_hh || !d->b_ih || !d->b_hh || !d->w1 || !d->b1 || !d->w2 || !d->b2 || !d->w3 || !d->b3) {
    d2d_set_error("%s: NULL parameter tensor", fn);
    return D2D_EINVAL;
  }
  return D2D_OK;
}

RdqnArgs make_args(const d2d_rdqn_desc* d, const float* obs, const uint8_t* rec, const uint32_t* sgn,
                   const int32_t* samples, int B, int shift) {
  RdqnArgs a = {};
  a.N = d->n_agents; a.E = d->n_envs; a.F = d->obs_dim; a.H = d->hidden; a.A = d->n_out;
  a.HT = (a.H + 15) / 16; a.IT = (a.F + 15) / 16;
  a.vecF = a.F % 4 == 0 && aligned16(d->w_ih);
  a.vecH = a.H % 4 == 0 && aligned16(d->w_hh) && aligned16(d->w1) && aligned16(d->w2) && aligned16(d->w3);
  a.w_ih = d->w_ih; a.w_hh = d->w_hh; a.b_ih = d->b_ih; a.b_hh = d->b_hh;
  a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2; a.b2 = d->b2; a.w3 = d->w3; a.b3 = d->b3;
  a.obs = obs; a.rec = rec; a.sgn = sgn; a.RB = D2D_RECORD_BYTES(a.F);
  a.rows = d->ring_rows; a.ep_len = d->ring_episode; a.shift = shift;
  a.ntrans = a.ep_len > 0 ? a.rows / (a.ep_len + 1) * a.ep_len : 0;
  a.samples = samples; a.B = B; a.mask_bytes = a.A <= 8 ? 1 : 2;
  a.seed = d->seed; a.env_base = d->env_base; a.rng_off = d->rng_offset;
  return a;
}

// obs_format_args with the entry point's name in front of its error text
int obs_args(const char* fn, int32_t format, const uint32_t* sgn_in, int32_t obs_dim, const void* obs, const float*& f32,
             const uint8_t*& rec, const uint32_t*& sgn) {
  const int rc = obs_format_args(format, sgn_in, obs_dim, obs, f32, rec, sgn);
  if (rc) {
    const std::string why = d2d_last_error();
    d2d_set_error("%s: %s", fn, why.c_str());
  }
  return rc;
}

}  // namespace
}  // namespace d2d

using namespace d2d;

extern "C" int64_t d2d_rdqn_carry_floats(const d2d_rdqn_desc* d, int32_t B) {
  if (!d || B < 0 || d->n_agents < 0 || d->hidden < 1 || d->hidden > 16 * kMaxHT) return -1;
  return (int64_t)d->n_agents * (16 * (((int64_t)B + 15) / 16)) * (16 * ((d->hidden + 15) / 16));
}

extern "C" int d2d_rdqn_q_ex(const d2d_rdqn_desc* d, const void* obs, int32_t obs_format, const uint32_t* obs_signed,
                             const int32_t* samples, int32_t B, int32_t row_shift, int32_t mode, float eps,
                             const float* eps_rows, int32_t ready, const uint8_t* explore_mask,
                             const uint8_t* explore_action, uint32_t rng_step, float* hcarry, int32_t carry_in,
                             float* q, float* qmax, void* action, void* stream) {
  const char* fn = "d2d_rdqn_q";
  int rc = check_desc(d, fn);
  if (rc) return rc;
  if (!obs || !samples || B < 0 || row_shift < 0 || row_shift > 1) {
    d2d_set_error("d2d_rdqn_q: NULL obs / samples, negative B or row_shift outside {0, 1}");
    return D2D_EINVAL;
  }
  const float* f32;
  const uint8_t* rec;
  const uint32_t* sgn;
  rc = obs_args(fn, obs_format, obs_signed, d->obs_dim, obs, f32, rec, sgn);
  if (rc) return rc;
  if (mode < D2D_RDQN_GREEDY || mode > D2D_RDQN_FORCED) { d2d_set_error("d2d_rdqn_q: unknown mode %d", mode); return D2D_EINVAL; }
  if (mode == D2D_RDQN_FORCED && action && (!explore_mask || !explore_action)) {
    d2d_set_error("d2d_rdqn_q: forced mode needs explore_mask and explore_action");
    return D2D_EINVAL;
  }
  if (mode == D2D_RDQN_EPS && !(eps >= 0.f && eps <= 1.f)) { d2d_set_error("d2d_rdqn_q: eps outside [0, 1]"); return D2D_EINVAL; }
  if (carry_in && !hcarry) { d2d_set_error("d2d_rdqn_q: carry_in needs hcarry"); return D2D_EINVAL; }
  if (carry_in && row_shift != 0) { d2d_set_error("d2d_rdqn_q: carry_in needs row_shift 0"); return D2D_EINVAL; }
  if (hcarry && !aligned16(hcarry)) { d2d_set_error("d2d_rdqn_q: hcarry must be 16-byte aligned"); return D2D_EINVAL; }
  if (B == 0 || d->n_agents == 0) return D2D_OK;
  RdqnArgs a = make_args(d, f32, rec, sgn, samples, B, row_shift);
  a.mode = mode; a.ready = ready ? 1 : 0; a.eps = eps; a.eps_rows = eps_rows; a.explore_mask = explore_mask; a.explore_action = explore_action;
  a.rng_step = rng_step; a.q = q; a.qmax = qmax; a.action = action;
  a.hcarry = hcarry; a.carry_in = carry_in ? 1 : 0;
  dim3 grid((B + 15) / 16, a.N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (rec && hcarry) hipLaunchKernelGGL((rdqn_q_kernel<true, true>), grid, dim3(64), 0, s, a);
  else if (rec) hipLaunchKernelGGL((rdqn_q_kernel<true, false>), grid, dim3(64), 0, s, a);
  else if (hcarry) hipLaunchKernelGGL((rdqn_q_kernel<false, true>), grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL((rdqn_q_kernel<false, false>), grid, dim3(64), 0, s, a);
  D2D_CHECK_HIP(hipGetLastError());
  return D2D_OK;
}

extern "C" int d2d_rdqn_q(const d2d_rdqn_desc* d, const float* obs, const int32_t* samples, int32_t B,
                          int32_t row_shift, int32_t mode, float eps, const float* eps_rows, int32_t ready,
                          const uint8_t* explore_mask, const uint8_t* explore_action, uint32_t rng_step, float* q, float* qmax, void* action,
                          void* stream) {
  return d2d_rdqn_q_ex(d, obs, D2D_OBS_F32, nullptr, samples, B, row_shift, mode, eps, eps_rows, ready, explore_mask,
                       explore_action, rng_step, nullptr, 0, q, qmax, action, stream);
}

extern "C" int64_t d2d_rdqn_grad_workspace(const d2d_rdqn_desc* d, int32_t B, int32_t L) {
  if (!d || B < 0 || L < 1 || L > kMaxWindow || d->n_agents < 0 || d->hidden < 1 || d->hidden > 16 * kMaxHT ||
      d->obs_dim < 1 || d->obs_dim + 1 > 16 * kMaxIT)
    return -1;
  return ws_layout(d->n_agents, L, B, (d->hidden + 15) / 16, (d->obs_dim + 15) / 16).total;
}

extern "C" int d2d_rdqn_grad_ex(const d2d_rdqn_desc* d, const void* obs, int32_t obs_format,
                                const uint32_t* obs_signed, const int32_t* samples, int32_t B, int32_t L,
                                const void* action, const float* reward, const uint8_t* done,
                                const float* qmax_target, float gamma, int32_t loss_kind, float* g_w_ih, float* g_w_hh,
                                float* g_b_ih, float* g_b_hh, float* g_w1, float* g_b1, float* g_w2, float* g_b2,
                                float* g_w3, float* g_b3, float* loss, float* workspace, int64_t workspace_floats,
                                void* stream) {
  const char* fn = "d2d_rdqn_grad";
  int rc = check_desc(d, fn);
  if (rc) return rc;
  if (L < 1 || L > kMaxWindow) {
    d2d_set_error("d2d_rdqn_grad: supports window lengths in [1, %d] (got %d)", kMaxWindow, L);
    return D2D_EUNSUPPORTED;
  }
  if (loss_kind != D2D_RDQN_HUBER && loss_kind != D2D_RDQN_MSE) {
    d2d_set_error("d2d_rdqn_grad: unknown loss %d", loss_kind);
    return D2D_EINVAL;
  }
  if (!obs || !samples || !action || !reward || !done || !qmax_target || !g_w_ih || !g_w_hh || !g_b_ih || !g_b_hh ||
      !g_w1 || !g_b1 || !g_w2 || !g_b2 || !g_w3 || !g_b3 || !loss || !workspace || B < 1) {
    d2d_set_error("d2d_rdqn_grad: NULL buffer or B < 1");
    return D2D_EINVAL;
  }
  const float* f32;
  const uint8_t* rec;
  const uint32_t* sgn;
  rc = obs_args(fn, obs_format, obs_signed, d->obs_dim, obs, f32, rec, sgn);
  if (rc) return rc;
  const WsLayout w = ws_layout(d->n_agents, L, B, (d->hidden + 15) / 16, (d->obs_dim + 15) / 16);
  if (workspace_floats < w.total || !aligned16(workspace)) {
    d2d_set_error("d2d_rdqn_grad: workspace of %lld floats, d2d_rdqn_grad_workspace asks for %lld (16-byte aligned)",
                  (long long)workspace_floats, (long long)w.total);
    return D2D_EINVAL;
  }
  if (d->n_agents == 0) return D2D_OK;
  RdqnArgs a = make_args(d, f32, rec, sgn, samples, B, 0);
  a.L = L; a.ntiles = (B + 15) / 16; a.huber = loss_kind == D2D_RDQN_HUBER; a.gamma = gamma;
  a.act_in = action; a.reward = reward; a.done = done; a.qmax_target = qmax_target;
  a.g_w_ih = g_w_ih; a.g_w_hh = g_w_hh; a.g_b_ih = g_b_ih; a.g_b_hh = g_b_hh; a.g_w1 = g_w1; a.g_b1 = g_b1;
  a.g_w2 = g_w2; a.g_b2 = g_b2; a.g_w3 = g_w3; a.g_b3 = g_b3; a.loss = loss;
  a.ws_x = workspace + w.x; a.ws_h = workspace + w.h; a.ws_g = workspace + w.g; a.ws_y1 = workspace + w.y1;
  a.ws_y2 = workspace + w.y2; a.ws_d1 = workspace + w.d1; a.ws_d2 = workspace + w.d2; a.ws_dq = workspace + w.dq;
  a.ws_loss = workspace + w.loss;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (rec) hipLaunchKernelGGL(rdqn_bptt_kernel<true>, dim3(a.ntiles, a.N), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(rdqn_bptt_kernel<false>, dim3(a.ntiles, a.N), dim3(64), 0, s, a);
  D2D_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(rdqn_wgrad_kernel, dim3(wgrad_tiles(a.HT, a.IT), a.N), dim3(64), 0, s, a);
  D2D_CHECK_HIP(hipGetLastError());
  return D2D_OK;
}

extern "C" int d2d_rdqn_grad(const d2d_rdqn_desc* d, const float* obs, const int32_t* samples, int32_t B, int32_t L,
                             const void* action, const float* reward, const uint8_t* done, const float* qmax_target,
                             float gamma, int32_t loss_kind, float* g_w_ih, float* g_w_hh, float* g_b_ih,
                             float* g_b_hh, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* g_w3,
                             float* g_b3, float* loss, float* workspace, int64_t workspace_floats, void* stream) {
  return d2d_rdqn_grad_ex(d, obs, D2D_OBS_F32, nullptr, samples, B, L, action, reward, done, qmax_target, gamma,
                          loss_kind, g_w_ih, g_w_hh, g_b_ih, g_b_hh, g_w1, g_b1, g_w2, g_b2, g_w3, g_b3, loss, workspace,
                          workspace_floats, stream);
}
