// Shared device/host helpers for the gfx950 kernels (wave64, CDNA4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "d2d_hip.h"

namespace d2d {

constexpr int kWave = 64;  // CDNA wavefront: every ballot below is 64-bit

enum : uint32_t { kStreamFlip = 0, kStreamArrival = 1, kStreamAction = 2, kPerEnv = 0xFFFFFFFFu };

struct u32x4 {
  uint32_t x, y, z, w;
};

// Philox4x32-10 (Salmon et al., SC'11); identical to oracle/philox.py and
// oracle/c/d2d_oracle.c, pinned to the Random123 known-answer vectors.
__device__ __forceinline__ u32x4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint64_t seed) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    // one 32x32->64 multiply per product (v_mad_u64_u32) gives both halves
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    // three-input xor in one v_bitop3_b32 (the compiler emits two v_xor_b32; the key words are
    // kernel-argument uniform, hence SGPR operands): comb step 65.4 -> 62.7 us at 64 x 8 x 65,536
    uint32_t n0, n2;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n0) : "v"((uint32_t)(p1 >> 32)), "v"(c1), "s"(k0));
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n2) : "v"((uint32_t)(p0 >> 32)), "v"(c3), "s"(k1));
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
  }
  return {c0, c1, c2, c3};
}

// philox() for the blocks of one lane whose counter words c0 and c2 (and the seed) are wave-uniform and
// whose word c1 is the lane's: the env kernels' (env, agent, step, stream | block) with one env per wave.
// A round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), so with
// U = wave-uniform and V = per-lane the words go (U, V, U, U) -> (V, U, U, U) -> (U, U, V, V) -> (V, V, V, U):
// both products of round 1, M1 c2 of round 2 and M0 c0 of round 3 are uniform, and the two per-lane products
// of rounds 2 and 3 do not depend on c3, so the blocks of a lane share them.  philox_head_of() computes what
// the blocks share once; philox_tail() finishes the block of counter word c3 = w3 (uniform).  Rounds 1-3 are
// plain C++, so that the compiler keeps every uniform value in scalar registers (the "v" operands of the
// v_bitop3 statements would force them into vector ones); rounds 4-10 are philox()'s.  Bit-identical to
// philox(c0, c1, c2, c3, seed): per block 14 of the 20 per-lane multiplies remain, plus the 2 shared ones.
struct philox_head {
  uint32_t y1;    // U: lo(M1 c2), word 1 after round 1
  uint32_t hi0;   // U: hi(M0 c0); word 2 after round 1 is hi0 ^ c3 ^ k1
  uint32_t z3;    // V: word 3 after round 2
  uint32_t r1hi, r1lo;  // V: the round-3 product M1 * (word 2 after round 2)
};

__device__ __forceinline__ philox_head philox_head_of(uint32_t c0, uint32_t c1, uint32_t c2, uint64_t seed) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0;  // U
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;  // U
  const uint32_t x0 = c1 ^ ((uint32_t)(p1 >> 32) ^ k0);  // V: word 0 after round 1
  const uint64_t q0 = (uint64_t)0xD2511F53u * x0;  // V, round 2
  const uint32_t z2 = (uint32_t)(q0 >> 32) ^ ((uint32_t)p0 ^ (k1 + 0xBB67AE85u));  // V: word 2 after round 2
  const uint64_t r1 = (uint64_t)0xCD9E8D57u * z2;  // V, round 3
  return {(uint32_t)p1, (uint32_t)(p0 >> 32), (uint32_t)q0, (uint32_t)(r1 >> 32), (uint32_t)r1};
}

__device__ __forceinline__ u32x4 philox_tail(const philox_head& h, uint32_t w3, uint64_t seed) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t c2_1 = h.hi0 ^ w3 ^ k1;  // U: word 2 after round 1
  k0 += 0x9E3779B9u;
  k1 += 0xBB67AE85u;
  const uint64_t q1 = (uint64_t)0xCD9E8D57u * c2_1;  // U, round 2
  const uint32_t c0_2 = (uint32_t)(q1 >> 32) ^ h.y1 ^ k0;  // U
  k0 += 0x9E3779B9u;
  k1 += 0xBB67AE85u;
  const uint64_t r0 = (uint64_t)0xD2511F53u * c0_2;  // U, round 3
  uint32_t c0 = h.r1hi ^ ((uint32_t)q1 ^ k0);
  uint32_t c1 = h.r1lo;
  uint32_t c2 = h.z3 ^ ((uint32_t)(r0 >> 32) ^ k1);
  uint32_t c3u = (uint32_t)r0;  // U: word 3 after round 3
  // round 4: word 3 is still uniform, its xor with the key stays scalar
  k0 += 0x9E3779B9u;
  k1 += 0xBB67AE85u;
  uint32_t c3;
  {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n0) : "v"((uint32_t)(p1 >> 32)), "v"(c1), "s"(k0));
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = (uint32_t)(p0 >> 32) ^ (c3u ^ k1);
    c3 = (uint32_t)p0;
  }
#pragma unroll
  for (int r = 4; r < 10; ++r) {
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0, n2;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n0) : "v"((uint32_t)(p1 >> 32)), "v"(c1), "s"(k0));
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n2) : "v"((uint32_t)(p0 >> 32)), "v"(c3), "s"(k1));
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
  }
  return {c0, c1, c2, c3};
}

__device__ __forceinline__ uint32_t pick(const u32x4& r, int i) {
  return i == 0 ? r.x : (i == 1 ? r.y : (i == 2 ? r.z : r.w));
}

// Poisson(lam) draw of word r: the sequential CDF inversion "x = 0, p = F = exp(-lam); while
// u >= F and x < 255: x += 1, p = p * lam / x, F += p" of u = r * 2^-32 (capped at 255, the uint8
// buffer cells), evaluated as a search of the agent's precomputed thresholds
// t[x] = ceil(F_x * 2^32) - 1 (d2d_env_desc.poisson_cdf, built on the host in the same IEEE double
// order): u >= F_x <=> r > t[x], t is nondecreasing and t[255] = 2^32 - 1, so the result is the
// count of leading entries below r -- bitwise the division loop, at four compares per 16-byte load
// instead of a double division per step.  x: the entries already counted (all below r, a multiple of 4), for a
// caller that compared the head of the row from a copy of its own.
__device__ __forceinline__ uint32_t poisson_lookup(uint32_t r, const uint32_t* __restrict__ t, uint32_t x = 0) {
  for (;;) {
    const uint4 q = *reinterpret_cast<const uint4*>(t + x);
    const uint32_t n = (uint32_t)(r > q.x) + (uint32_t)(r > q.y) + (uint32_t)(r > q.z) + (uint32_t)(r > q.w);
    x += n;
    if (n < 4u) return x;
  }
}

}  // namespace d2d

// thread-local last-error string for the C ABI
void d2d_set_error(const char* fmt, ...);

#define D2D_CHECK_HIP(expr)                                                    \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      d2d_set_error("%s: %s", #expr, hipGetErrorString(_e));                   \
      return D2D_EHIP;                                                         \
    }                                                                          \
  } while (0)

// obs_format of a d2d_mlp_desc / d2d_gru_desc: the obs argument as fp32 rows (f32) or as the
// env kernel's compact record (rec, with the int8-column masks sgn); exactly one is set
inline int obs_format_args(int32_t format, const uint32_t* sgn_in, int32_t obs_dim, const void* obs, const float*& f32,
                           const uint8_t*& rec, const uint32_t*& sgn) {
  f32 = nullptr; rec = nullptr; sgn = nullptr;
  if (format == D2D_OBS_F32) { f32 = static_cast<const float*>(obs); return D2D_OK; }
  if (format != D2D_OBS_U8) { d2d_set_error("unknown obs_format %d", format); return D2D_EINVAL; }
  if (!sgn_in) { d2d_set_error("obs_format D2D_OBS_U8 needs obs_signed"); return D2D_EINVAL; }
  if (reinterpret_cast<uintptr_t>(obs) & 15) { d2d_set_error("the obs record must be 16-byte aligned"); return D2D_EINVAL; }
  (void)obs_dim;
  rec = static_cast<const uint8_t*>(obs); sgn = sgn_in;
  return D2D_OK;
}
