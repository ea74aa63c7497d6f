// GRU pieces for hidden sizes up to 128, shared by the iRDQN kernels (rdqn_kernels.hip) and the wide PPO GRU kernels
// (gru_wide_kernels.hip).  The layout is the one rdqn_kernels.hip describes: v_mfma_f32_16x16x4_f32, one 16-sample
// tile per wave and one wave per workgroup, every layer transposed; vectors live in LDS as "vector images"
// V[tile][lane] of f32x4 in accumulator layout, weight fragments come straight from the agent-stacked tensors in
// global memory (L2-resident), and rows / columns past H, F or A read as exact zeros.  Every product is exact fp32.
//
// The helpers that read the launch arguments are templates on the argument struct; they use its fields
//   H, F, HT, IT, vecF, vecH, w_ih, w_hh, b_ih, b_hh      (gru_step, dense)
//   RB, sgn                                               (RecSigns)
#pragma once
#include "common.h"
#include "gru_common.h"

namespace d2d {

constexpr int kMaxHT = 8, kMaxIT = 4, kMaxWindow = 256;

// W[row][col .. col + 3] of a [rows][cols] matrix, zeros outside (col % 4 == 0)
__device__ __forceinline__ f32x4 wfrag(const float* W, int rows, int cols, int row, int col, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row < rows && col < cols) {
    const float* p = W + (size_t)row * cols + col;
    if (vec) {
      v = *reinterpret_cast<const f32x4*>(p);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (col + r < cols) v[r] = p[r];
    }
  }
  return v;
}

// b[u0 .. u0 + 3] of an n-vector, zeros outside
__device__ __forceinline__ f32x4 bfrag(const float* b, int n, int u0) {
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = u0 + r < n ? b[u0 + r] : 0.f;
  return v;
}

// one wave per workgroup: LDS writes of one lane become visible to the others
__device__ __forceinline__ void wave_sync() { __syncthreads(); }

// acc += W[16t + (4g + r)][..] . v for the [rows][cols] matrix W and the vector image v of `kt` k-tiles
__device__ __forceinline__ f32x4 mat_vec(f32x4 acc, const float* W, int rows, int cols, bool vec, int t,
                                         const f32x4* v, int kt, int lane) {
  const int g = lane >> 4, i = lane & 15;
  for (int q = 0; q < kt; ++q) {
    const f32x4 wv = wfrag(W, rows, cols, 16 * t + i, 16 * q + 4 * g, vec);
    const f32x4 xv = v[q * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc = mfma4(wv[r], xv[r], acc);
  }
  return acc;
}

// acc += (W^T d)[16t' + (4g + r)] for the [rows][cols] matrix W and the image d of `rt` row tiles
__device__ __forceinline__ f32x4 mat_t_vec(f32x4 acc, const float* W, int rows, int cols, int tp, const f32x4* d,
                                           int rt, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const int c = 16 * tp + i;
  for (int T = 0; T < rt; ++T) {
    const f32x4 dv = d[T * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int R = 16 * T + 4 * g + r;
      const float a = (R < rows && c < cols) ? W[(size_t)R * cols + c] : 0.f;
      acc = mfma4(a, dv[r], acc);
    }
  }
  return acc;
}

// agent k's int8-column masks of the record (workgroup-uniform: scalar registers, as XSigns of gru_common.h);
// RB <= 64, so two words.  REC: the kernel instance that reads the record -- the fp32 instances carry none of this.
template <bool REC>
struct RecSigns {
  uint32_t w[2];
  template <class Args>
  __device__ __forceinline__ RecSigns(const Args& a, int k) {
    w[0] = w[1] = 0u;
    if constexpr (REC) {
      const int nw = a.RB >> 5;
      w[0] = __builtin_amdgcn_readfirstlane(a.sgn[(size_t)k * nw]);
      if (nw > 1) w[1] = __builtin_amdgcn_readfirstlane(a.sgn[(size_t)k * nw + 1]);
    }
  }
  // flags of columns col .. col + 3 (col % 4 == 0, col < 64)
  __device__ __forceinline__ uint32_t bits4(int col) const { return ((col < 32 ? w[0] : w[1]) >> (col & 31)) & 0xFu; }
};

// One GRU step of agent k on the images xs / hs -> hn.  active: this lane's sample is inside its window (else its h
// stays 0).  gates != nullptr: r, z, n and W_hn h + b_hn go to gates[G * HW + unit] of this lane's sample.
template <class Args>
__device__ __forceinline__ void gru_step(const Args& a, int k, const f32x4* xs, const f32x4* hs, f32x4* hn,
                                         bool h_zero, bool active, float* gates, int lane) {
  const int g = lane >> 4, H = a.H, F = a.F, HW = 16 * a.HT;
  const float* Wih = a.w_ih + (size_t)k * 3 * H * F;
  const float* Whh = a.w_hh + (size_t)k * 3 * H * H;
  const float* bih = a.b_ih + (size_t)k * 3 * H;
  const float* bhh = a.b_hh + (size_t)k * 3 * H;
  for (int t = 0; t < a.HT; ++t) {
    const int u0 = 16 * t + 4 * g;
    f32x4 ar = bfrag(bih, H, u0) + bfrag(bhh, H, u0);
    f32x4 az = bfrag(bih + H, H, u0) + bfrag(bhh + H, H, u0);
    f32x4 ani = bfrag(bih + 2 * H, H, u0);
    f32x4 anh = bfrag(bhh + 2 * H, H, u0);
    ar = mat_vec(ar, Wih, H, F, a.vecF, t, xs, a.IT, lane);
    az = mat_vec(az, Wih + (size_t)H * F, H, F, a.vecF, t, xs, a.IT, lane);
    ani = mat_vec(ani, Wih + (size_t)2 * H * F, H, F, a.vecF, t, xs, a.IT, lane);
    if (!h_zero) {
      ar = mat_vec(ar, Whh, H, H, a.vecH, t, hs, a.HT, lane);
      az = mat_vec(az, Whh + (size_t)H * H, H, H, a.vecH, t, hs, a.HT, lane);
      anh = mat_vec(anh, Whh + (size_t)2 * H * H, H, H, a.vecH, t, hs, a.HT, lane);
    }
    const f32x4 ho = hs[t * 64 + lane];
    f32x4 hv, rv, zv, nv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      rv[r] = sigmoidf_(ar[r]);
      zv[r] = sigmoidf_(az[r]);
      nv[r] = gru_n(ani[r], rv[r], anh[r]);
      hv[r] = active ? fmaf(zv[r], ho[r] - nv[r], nv[r]) : 0.f;  // (1 - z) n + z h
    }
    hn[t * 64 + lane] = hv;
    if (gates) {
      *reinterpret_cast<f32x4*>(gates + u0) = rv;
      *reinterpret_cast<f32x4*>(gates + HW + u0) = zv;
      *reinterpret_cast<f32x4*>(gates + 2 * HW + u0) = nv;
      *reinterpret_cast<f32x4*>(gates + 3 * HW + u0) = anh;
    }
  }
}

// out = W v + b (relu: max(., 0)) for a [rows][H] layer; out has `ot` tiles
template <class Args>
__device__ __forceinline__ void dense(const Args& a, const float* W, const float* b, int rows, int ot,
                                      const f32x4* v, f32x4* out, bool relu_, int lane) {
  const int g = lane >> 4;
  for (int t = 0; t < ot; ++t) {
    f32x4 acc = bfrag(b, rows, 16 * t + 4 * g);
    acc = mat_vec(acc, W, rows, a.H, a.vecH, t, v, a.HT, lane);
    if (relu_) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = relu(acc[r]);
    }
    out[t * 64 + lane] = acc;
  }
}

// out[16 Tm + 4g + r][16 Tn + i] = sum_k A[k][16 Tm + ..] B[k][16 Tn + ..] (Bm == nullptr: B = 1), k in order
__device__ __forceinline__ f32x4 outer_tile(const float* A, int lda, const float* Bm, int ldb, int K, int lane) {
  const int g = lane >> 4, i = lane & 15;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* pa = A + (size_t)g * lda + i;
  const float* pb = Bm ? Bm + (size_t)g * ldb + i : nullptr;
  for (int k0 = 0; k0 < K; k0 += 16) {  // K is a multiple of 16 (whole sample tiles): four loads in flight
    float av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      av[s] = pa[(size_t)(k0 + 4 * s) * lda];
      bv[s] = pb ? pb[(size_t)(k0 + 4 * s) * ldb] : 1.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = mfma4(av[s], bv[s], acc);
  }
  return acc;
}

// rows [r0, r0 + 4) x column c of a [rows][cols] gradient tensor
__device__ __forceinline__ void store_tile(float* out, int rows, int cols, int r0, int c, f32x4 v) {
  if (c >= cols) return;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r0 + r < rows) out[(size_t)(r0 + r) * cols + c] = v[r];
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace d2d
