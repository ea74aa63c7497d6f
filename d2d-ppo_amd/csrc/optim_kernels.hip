// The parameter update for gfx950: per-agent gradient-norm clipping + Adam in one call (d2d_adam_step).
//
// Replaces torch.nn.utils.clip_grad_norm_ per agent followed by torch.optim.Adam.step() at its defaults
// (the reference's ippo.py:204-215, d2d_ppo.py:209-212 and 443-446, irdqn.py:144-146): the learners'
// StackedNets.grad_norm_clip_ (per tensor a pow, a sum and a mul_, plus a sqrt and a clamp) and a foreach Adam
// of about ten launches per optimizer become one launch without clipping and three with it.
//
// Every tensor of the table is agent-stacked, [n_agents][numel] contiguous, so for the element-wise update it is ONE
// flat array of n_agents * numel floats: the update kernel walks that array in 16-byte groups from the first
// 16-byte aligned element on, whatever the per-agent slices' own alignment is (b2 [N][8], w1 [N][5][3]: odd agents
// start unaligned; the flat array does not care), the up-to-3 head elements and the ragged tail as scalars.  A group
// that straddles two agents looks its clip coefficients up per element.  param, grad, exp_avg and exp_avg_sq must
// share their address modulo 16 for the 16-byte path; a table entry where they do not takes scalar accesses.
//
// The norm is the only reduction.  Its order is fixed by the slice index alone (never by an address), and nothing is
// accumulated with atomics, so equal inputs give equal bits at any alignment:
//   adam_norm_partial   grid (P, n_agents): block (p, k) sums g^2 over one chunk of kNormChunk elements of one
//                       tensor of agent k -- lane l takes elements l, l + 256, ... in double (a float's square is
//                       exact there), then a fixed shuffle / LDS tree -- and writes one double partial [k][p];
//   adam_norm_finalize  one wave per agent: the P partials strided over the lanes, a fixed tree, norm = (float)sqrt
//                       (one rounding of the double sum, so coef is good to a roundoff for a 128 x 3,848 central-critic
//                       w1 as for a 2-element bias), coef = min(1, max_norm / (norm + 1e-6)) in fp32 as torch does;
//                       it also advances the device step counter, which the update then reads;
//   adam_update         g <- coef g (written back where coef < 1), then Adam, element-wise in fp32 as written
//                       (-ffp-contract=off; hipcc's fp32 sqrt and divide are correctly rounded by default).
// Without clipping and with a host step the call is adam_update alone; a device step counter without clipping adds a
// one-thread launch that advances it (the update's workgroups cannot both read and advance one word without a race).
#include <cmath>

#include "common.h"

namespace d2d {

constexpr int kAdamThreads = 256;
constexpr int kAdamGroups = 2;                                 // 16-byte groups per lane
constexpr int kAdamChunk = kAdamThreads * 4 * kAdamGroups;     // elements per workgroup of the update
constexpr int kNormChunk = 4096;                               // elements per norm partial

struct AdamTensor {
  float *p, *g, *m, *v;
  int64_t total, numel;  // n_agents * numel, numel
  int32_t head, vec;     // scalar elements before the first 16-byte group; 0: scalar accesses throughout
};

// the tensor table and the first workgroup (update) or first chunk (norm) of every tensor, by value in the arguments
struct AdamTable {
  AdamTensor t[D2D_ADAM_MAX_TENSORS];
  int32_t first[D2D_ADAM_MAX_TENSORS + 1];
  int32_t n;
};

struct AdamScalars {
  float w1, b2, w2, eps, step_size, bc2s;  // 1 - beta1, beta2, 1 - beta2; step_size, bc2s: host step only
  double lr, beta1, beta2;
  const int64_t* step_dev;
  const float* coef;                       // [n_agents], NULL without clipping
  int32_t n_agents;
};

__device__ __forceinline__ int adam_find(const AdamTable& tab, int b) {
  int ti = 0;
  while (ti + 1 < tab.n && b >= tab.first[ti + 1]) ++ti;
  return ti;
}

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& s) {
  m = m + (g - m) * s.w1;                          // exp_avg.lerp_(grad, 1 - beta1)
  v = s.b2 * v + (s.w2 * g) * g;                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / s.bc2s + s.eps;   // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  p = p - s.step_size * (m / denom);               // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(kAdamThreads) void adam_update_kernel(AdamTable tab, AdamScalars s) {
  const int ti = adam_find(tab, (int)blockIdx.x);
  const AdamTensor& T = tab.t[ti];
  const int64_t lb = (int64_t)blockIdx.x - tab.first[ti];
  const int tid = threadIdx.x;
  if (s.step_dev) {  // the counter was advanced by the launch before this one
    const double t = (double)*s.step_dev;
    s.bc2s = (float)sqrt(1.0 - pow(s.beta2, t));
    s.step_size = (float)(s.lr / (1.0 - pow(s.beta1, t)));
  }
  const bool clip = s.coef != nullptr;
  const bool one = s.n_agents == 1;
  const bool small = T.total <= 0xFFFFFFFFll;
  auto agent_of = [&](int64_t e) -> int64_t {
    if (one) return 0;
    return small ? (int64_t)((uint32_t)e / (uint32_t)T.numel) : e / T.numel;
  };
  auto scalar_at = [&](int64_t e) {
    float g = T.g[e], p = T.p[e], m = T.m[e], v = T.v[e];
    if (clip) {
      const float c = s.coef[agent_of(e)];
      if (c != 1.f) {
        g = c * g;
        T.g[e] = g;
      }
    }
    adam_elem(p, g, m, v, s);
    T.p[e] = p;
    T.m[e] = m;
    T.v[e] = v;
  };
  if (lb == 0 && tid < T.head) scalar_at(tid);  // (head <= total, set on the host)
#pragma unroll
  for (int u = 0; u < kAdamGroups; ++u) {
    const int64_t e = T.head + lb * kAdamChunk + (int64_t)(u * kAdamThreads + tid) * 4;
    if (e >= T.total) continue;
    if (!T.vec || e + 4 > T.total) {
      for (int j = 0; j < 4; ++j)
        if (e + j < T.total) scalar_at(e + j);
      continue;
    }
    float4 g = *reinterpret_cast<const float4*>(T.g + e);
    float4 p = *reinterpret_cast<const float4*>(T.p + e);
    float4 m = *reinterpret_cast<const float4*>(T.m + e);
    float4 v = *reinterpret_cast<const float4*>(T.v + e);
    if (clip) {
      float c0, c1, c2, c3;
      const int64_t k = agent_of(e);
      if (one || e + 4 <= (k + 1) * T.numel) {
        c0 = c1 = c2 = c3 = s.coef[k];
      } else {  // the group straddles agents
        c0 = s.coef[k];
        c1 = s.coef[agent_of(e + 1)];
        c2 = s.coef[agent_of(e + 2)];
        c3 = s.coef[agent_of(e + 3)];
      }
      if (c0 != 1.f || c1 != 1.f || c2 != 1.f || c3 != 1.f) {
        g.x = c0 * g.x;
        g.y = c1 * g.y;
        g.z = c2 * g.z;
        g.w = c3 * g.w;
        *reinterpret_cast<float4*>(T.g + e) = g;
      }
    }
    adam_elem(p.x, g.x, m.x, v.x, s);
    adam_elem(p.y, g.y, m.y, v.y, s);
    adam_elem(p.z, g.z, m.z, v.z, s);
    adam_elem(p.w, g.w, m.w, v.w, s);
    *reinterpret_cast<float4*>(T.p + e) = p;
    *reinterpret_cast<float4*>(T.m + e) = m;
    *reinterpret_cast<float4*>(T.v + e) = v;
  }
}

// sum of the workgroup's doubles in a fixed order: shuffle tree inside each wave, then the waves' sums in order
__device__ __forceinline__ double adam_block_sum(double a, double* sh) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) a += __shfl_down(a, off, kWave);
  const int w = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) sh[w] = a;
  __syncthreads();
  double r = 0.0;
  for (int i = 0; i < (int)blockDim.x / kWave; ++i) r += sh[i];
  return r;
}

__global__ __launch_bounds__(kAdamThreads) void adam_norm_partial_kernel(AdamTable tab, int P, double* __restrict__ part) {
  __shared__ double sh[kAdamThreads / kWave];
  const int ti = adam_find(tab, (int)blockIdx.x);
  const AdamTensor& T = tab.t[ti];
  const int64_t k = blockIdx.y;
  const int64_t off = ((int64_t)blockIdx.x - tab.first[ti]) * kNormChunk;
  const int64_t left = T.numel - off;
  const int n = left < kNormChunk ? (int)left : kNormChunk;
  const float* __restrict__ g = T.g + k * T.numel + off;
  double a = 0.0;
#pragma unroll 4
  for (int i = threadIdx.x; i < n; i += kAdamThreads) {
    const double x = (double)g[i];
    a += x * x;
  }
  a = adam_block_sum(a, sh);
  if (threadIdx.x == 0) part[k * P + blockIdx.x] = a;
}

__global__ __launch_bounds__(kWave) void adam_norm_finalize_kernel(const double* __restrict__ part, int P, float max_norm,
                                                                   float* __restrict__ coef, float* __restrict__ grad_norm,
                                                                   int64_t* step_dev) {
  const int64_t k = blockIdx.x;
  double a = 0.0;
  for (int i = threadIdx.x; i < P; i += kWave) a += part[k * P + i];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) a += __shfl_down(a, off, kWave);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(a);
    // clip_grad_norm_: max_norm / (total_norm + 1e-6), clamped to 1; a NaN norm gives a NaN coefficient, as
    // torch.clamp does (fminf would return 1)
    const float c = max_norm / (norm + 1e-6f);
    coef[k] = c > 1.f ? 1.f : c;
    if (grad_norm) grad_norm[k] = norm;
    if (k == 0 && step_dev) *step_dev += 1;
  }
}

__global__ void adam_tick_kernel(int64_t* step_dev) { *step_dev += 1; }

}  // namespace d2d

using namespace d2d;

// every rule of the header, before any HIP call; P: norm partials per agent
static int adam_check(const d2d_adam_desc* d, const char* who, int64_t* P_out) {
  if (!d) { d2d_set_error("%s: NULL desc", who); return D2D_EINVAL; }
  if (d->n_tensors < 1 || d->n_tensors > D2D_ADAM_MAX_TENSORS) {
    d2d_set_error("%s: n_tensors %d outside [1, %d]", who, d->n_tensors, D2D_ADAM_MAX_TENSORS);
    return D2D_EINVAL;
  }
  if (d->n_agents < 0) { d2d_set_error("%s: negative n_agents %d", who, d->n_agents); return D2D_EINVAL; }
  int64_t P = 0;
  for (int i = 0; i < d->n_tensors; ++i) {
    const d2d_adam_tensor& t = d->tensors[i];
    if (t.numel < 0) { d2d_set_error("%s: tensor %d: negative numel %lld", who, i, (long long)t.numel); return D2D_EINVAL; }
    if (t.numel == 0) continue;
    if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) {
      d2d_set_error("%s: tensor %d: NULL param, grad, exp_avg or exp_avg_sq of a non-empty tensor", who, i);
      return D2D_EINVAL;
    }
    if ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) |
         reinterpret_cast<uintptr_t>(t.exp_avg) | reinterpret_cast<uintptr_t>(t.exp_avg_sq)) & 3) {
      d2d_set_error("%s: tensor %d: pointers must be 4-byte aligned", who, i);
      return D2D_EINVAL;
    }
    if (d->n_agents > 0 && t.numel > (int64_t)0x7FFFFFFFFFFFll / d->n_agents) {
      d2d_set_error("%s: tensor %d: n_agents * numel too large", who, i);
      return D2D_EINVAL;
    }
    P += (t.numel + kNormChunk - 1) / kNormChunk;
  }
  if (!d->step_dev && d->step < 1) {
    d2d_set_error("%s: step %lld < 1 without step_dev", who, (long long)d->step);
    return D2D_EINVAL;
  }
  if (!(d->beta1 >= 0.0 && d->beta1 < 1.0)) { d2d_set_error("%s: beta1 %g outside [0, 1)", who, d->beta1); return D2D_EINVAL; }
  if (!(d->beta2 >= 0.0 && d->beta2 < 1.0)) { d2d_set_error("%s: beta2 %g outside [0, 1)", who, d->beta2); return D2D_EINVAL; }
  if (!(d->eps >= 0.0)) { d2d_set_error("%s: eps %g < 0", who, d->eps); return D2D_EINVAL; }
  if (!(d->lr >= 0.0)) { d2d_set_error("%s: lr %g < 0", who, d->lr); return D2D_EINVAL; }
  if (P > 0x7FFFFFFF) { d2d_set_error("%s: too many norm partials", who); return D2D_EINVAL; }
  if (d->max_norm > 0.0 && d->n_agents > 65535) {  // one grid row per agent in the norm pass
    d2d_set_error("%s: clipping supports n_agents <= 65535, got %d", who, d->n_agents);
    return D2D_EUNSUPPORTED;
  }
  *P_out = P;
  return D2D_OK;
}

// [n_agents][P] double partials, then [n_agents] float coefficients
static int64_t adam_workspace_bytes(const d2d_adam_desc* d, int64_t P) {
  if (!(d->max_norm > 0.0) || d->n_agents == 0 || P == 0) return 0;
  return ((int64_t)d->n_agents * P * 8 + (int64_t)d->n_agents * 4 + 7) & ~(int64_t)7;
}

extern "C" int64_t d2d_adam_workspace(const d2d_adam_desc* desc) {
  int64_t P = 0;
  if (adam_check(desc, "d2d_adam_workspace", &P) != D2D_OK) return -1;
  return adam_workspace_bytes(desc, P);
}

extern "C" int d2d_adam_step(const d2d_adam_desc* desc, void* workspace, int64_t workspace_bytes, float* grad_norm,
                             void* stream) {
  int64_t P = 0;
  const int rc = adam_check(desc, "d2d_adam_step", &P);
  if (rc != D2D_OK) return rc;
  const int64_t need = adam_workspace_bytes(desc, P);
  if (need > 0) {
    if (!workspace || workspace_bytes < need) {
      d2d_set_error("d2d_adam_step: workspace NULL or too small: %lld bytes, d2d_adam_workspace asks for %lld",
                    (long long)(workspace ? workspace_bytes : 0), (long long)need);
      return D2D_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) {
      d2d_set_error("d2d_adam_step: workspace must be 8-byte aligned");
      return D2D_EINVAL;
    }
  }
  const int N = desc->n_agents;
  if (N == 0 || P == 0) return D2D_OK;  // nothing to update: no launch (the device step does not advance either)
  AdamTable upd{}, nrm{};
  int64_t blocks = 0, chunks = 0;
  int n = 0;
  for (int i = 0; i < desc->n_tensors; ++i) {
    const d2d_adam_tensor& t = desc->tensors[i];
    if (t.numel == 0) continue;
    AdamTensor& a = upd.t[n];
    a.p = t.param; a.g = t.grad; a.m = t.exp_avg; a.v = t.exp_avg_sq;
    a.numel = t.numel;
    a.total = t.numel * N;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(t.param) & 15;
    a.vec = lo == (reinterpret_cast<uintptr_t>(t.grad) & 15) && lo == (reinterpret_cast<uintptr_t>(t.exp_avg) & 15) &&
            lo == (reinterpret_cast<uintptr_t>(t.exp_avg_sq) & 15);
    a.head = a.vec ? (int32_t)(((16 - lo) & 15) / 4) : 0;
    if (a.head > a.total) a.head = (int32_t)a.total;
    nrm.t[n] = a;
    upd.first[n] = (int32_t)blocks;
    nrm.first[n] = (int32_t)chunks;
    const int64_t body = a.total - a.head;
    blocks += body > 0 ? (body + kAdamChunk - 1) / kAdamChunk : 1;
    chunks += (t.numel + kNormChunk - 1) / kNormChunk;
    if (blocks > 0x7FFFFFFF) { d2d_set_error("d2d_adam_step: too many elements for one launch"); return D2D_EUNSUPPORTED; }
    ++n;
  }
  upd.first[n] = (int32_t)blocks;
  nrm.first[n] = (int32_t)chunks;
  upd.n = nrm.n = n;
  const bool clip = need > 0;
  AdamScalars s{};
  s.w1 = (float)(1.0 - desc->beta1);
  s.b2 = (float)desc->beta2;
  s.w2 = (float)(1.0 - desc->beta2);
  s.eps = (float)desc->eps;
  s.lr = desc->lr; s.beta1 = desc->beta1; s.beta2 = desc->beta2;
  s.step_dev = desc->step_dev;
  s.n_agents = N;
  if (!desc->step_dev) {  // as torch does on the host: in double, rounded to float once
    const double t = (double)desc->step;
    s.bc2s = (float)std::sqrt(1.0 - std::pow(desc->beta2, t));
    s.step_size = (float)(desc->lr / (1.0 - std::pow(desc->beta1, t)));
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (clip) {
    double* part = static_cast<double*>(workspace);
    float* coef = reinterpret_cast<float*>(part + (int64_t)N * P);
    hipLaunchKernelGGL(adam_norm_partial_kernel, dim3((unsigned)P, (unsigned)N), dim3(kAdamThreads), 0, st, nrm, (int)P, part);
    D2D_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(adam_norm_finalize_kernel, dim3((unsigned)N), dim3(kWave), 0, st, part, (int)P,
                       (float)desc->max_norm, coef, grad_norm, desc->step_dev);
    D2D_CHECK_HIP(hipGetLastError());
    s.coef = coef;
  } else if (desc->step_dev) {
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, st, desc->step_dev);
    D2D_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(adam_update_kernel, dim3((unsigned)blocks), dim3(kAdamThreads), 0, st, upd, s);
  D2D_CHECK_HIP(hipGetLastError());
  return D2D_OK;
}
