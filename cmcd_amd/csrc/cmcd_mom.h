// What the reverse-time chains and the chain segments of the two momentum baselines share (cmcd_reverse_ldvi.hip,
// cmcd_reverse_hais.hip, cmcd_segment_ldvi.hip, cmcd_segment_hais.hip): the geffner
// score network on [z; rho] for 16 particles per wave, the log density of a standard-normal momentum, a uniform value moved to
// a scalar register, and Hamiltonian AIS's beta table formed from params_flat in the workgroup prologue.
//
// mom_pre_z / mom_eval_rho are the geffner branch of cmcd_uha.hip's net_pre_z / net_eval_rho, as cmcd_ldvi.hip's ldvi_pre_z /
// ldvi_eval_rho are (cmcd_tile.h lists the copies and why they are copies: cmcd_uha.hip is hashed for the stored counter
// figures, cmcd_ldvi.hip and cmcd_reverse_uha.hip stay as they are).  tests/test_gpu_reverse_ldvi.py's parity cases on all
// three widths fail when this copy drifts.  mom_form_betas is cmcd_hais.hip's hais_form_betas with the layout and K handed in.
#pragma once
#include "cmcd_tile.h"

namespace cmcd {

// a value every lane of the wave holds alike (a parameter, a schedule entry), moved to a scalar register
__device__ __forceinline__ float mom_uniform(float v) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

// log N(rho; 0, I)
template <int D>
__device__ __forceinline__ float mom_log_n01(const float (&rho)[D]) {
  float l = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) l += -(rho[j] * rho[j]) * 0.5f - kHalfLog2Pi;
  return l;
}

// first-layer pre-activation of the z part: bias row (embedding folded by the prep launch) + z W1[:d]
template <int D, int T>
__device__ __forceinline__ void mom_pre_z(const float (&z)[D], const float* __restrict__ brow, const float* lds_w1z, int g,
                                          f32x4 (&pre)[T]) {
  constexpr int HP = 16 * T;
  asm volatile("" ::: "memory");  // keep the LDS-resident weights streaming (no LICM into VGPRs)
#pragma unroll
  for (int t = 0; t < T; ++t) {
    pre[t] = *reinterpret_cast<const f32x4*>(brow + 16 * t + 4 * g);
#pragma unroll
    for (int j = 0; j < D; ++j) pre[t] += z[j] * *reinterpret_cast<const f32x4*>(lds_w1z + j * HP + 16 * t + 4 * g);
  }
}

// s([z; rho], i) of the geffner net for the 16 particles of this wave
//   u = [z; rho; emb]; u += softplus(u W1 + b1); u += softplus(u W2 + b2); factor (u W3 + b3)      nn.py:45-52,66-70
template <int D, int T>
__device__ __forceinline__ void mom_eval_rho(const f32x4 (&prez)[T], const float (&z)[D], const float (&rho)[D],
                                             const float* __restrict__ urow, const float* lds_w2, const float* lds_w1z,
                                             const float* lds_b2, const float* lds_w3t, const float* lds_b3, int lane,
                                             float (&s)[D]) {
  constexpr int HP = 16 * T;
  const int g = lane >> 4;
  asm volatile("" ::: "memory");
  f32x4 h[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    f32x4 pre = prez[t];
#pragma unroll
    for (int j = 0; j < D; ++j) pre += rho[j] * *reinterpret_cast<const f32x4*>(lds_w1z + (D + j) * HP + 16 * t + 4 * g);
    f32x4 u = *reinterpret_cast<const f32x4*>(urow + 16 * t + 4 * g);
    if (16 * t < 2 * D) {  // the first 2 D entries of u are [z; rho] themselves
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nidx = 16 * t + 4 * g + r;
#pragma unroll
        for (int j = 0; j < D; ++j) {
          if (j >= 16 * t && j < 16 * t + 16) u[r] = (nidx == j) ? z[j] : u[r];
          if (D + j >= 16 * t && D + j < 16 * t + 16) u[r] = (nidx == D + j) ? rho[j] : u[r];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) h[t][r] = u[r] + softplus(pre[r]);
  }
  // layer 2 on the matrix cores: acc[to] rows = neurons 16 to + 4 g + r, columns = particles
  f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = *reinterpret_cast<const f32x4*>(lds_b2 + 16 * t + 4 * g);
#pragma unroll
  for (int ti = 0; ti < T; ++ti) {
    asm volatile("" ::: "memory");
    f32x4 af[T];
#pragma unroll
    for (int to = 0; to < T; ++to) af[to] = *reinterpret_cast<const f32x4*>(lds_w2 + ((ti * T + to) * 64 + lane) * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int to = 0; to < T; ++to) acc[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[to][r], h[ti][r], acc[to], 0, 0, 0);
    }
  }
  // layer 3: every lane sums over its 4 T neurons, then the 4 lanes of a particle combine
  float part[D];
#pragma unroll
  for (int j = 0; j < D; ++j) part[j] = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    f32x4 h2;
#pragma unroll
    for (int r = 0; r < 4; ++r) h2[r] = h[t][r] + softplus(acc[t][r]);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(lds_w3t + j * HP + 16 * t + 4 * g);
      part[j] += h2[0] * wv[0] + h2[1] * wv[1] + h2[2] * wv[2] + h2[3] * wv[3];
    }
  }
  const float factor = lds_b3[15];
#pragma unroll
  for (int j = 0; j < D; ++j) s[j] = (group_sum(part[j]) + lds_b3[j]) * factor;
}

// cell of np.interp for abscissa x on the grid gx[0 .. G + 1]: searchsorted(gx, x, side = 'right') clipped to [1, G + 1]
__device__ __forceinline__ int mom_cell(const float* gx, int G, float x) {
  int j = 1;
  while (j < G + 1 && gx[j] <= x) ++j;
  return j;
}

// Hamiltonian AIS: betas[K] = interp(target_x, gridref_x, [0, cumsum(mgridref_y) / sum]) into LDS, by the whole workgroup;
// gy[ngrid + 2] is scratch next to them.  Ends with a barrier.
__device__ __forceinline__ void mom_form_betas(const float* params, const cmcd_hais_layout& lay, int K, float* betas, float* gy) {
  const int G = (int)lay.ngrid;
  const float* m = params + lay.mgridref_y;
  const float* gx = params + lay.gridref_x;
  if (threadIdx.x == 0) {   // the running sum stays sequential: same association as a serial cumsum
    float run = 0.f;
    gy[0] = 0.f;
    for (int q = 0; q <= G; ++q) {
      run += m[q];
      gy[q + 1] = run;
    }
    for (int q = 1; q <= G + 1; ++q) gy[q] = gy[q] / run;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    const float x = params[lay.target_x + i];
    const int j = mom_cell(gx, G, x);
    betas[i] = gy[j - 1] + ((x - gx[j - 1]) / (gx[j] - gx[j - 1])) * (gy[j] - gy[j - 1]);
  }
  __syncthreads();
}

}  // namespace cmcd
