// The wave-per-tile chain machinery that cmcd_reverse.hip and cmcd_segment.hip share (included by nothing else): the score
// network on 16 particles per wave, a key split and one step of the key chain, the statistics butterflies, the instance table
// and the launch.  Each kernel file keeps its chain: direction, what opens and what closes a step, how it
// enters and leaves.
//
// This is the SECOND copy of that machinery, and a named one: traj_kernel (cmcd_kernels.hip) holds the first, with its debug
// outputs and ablation probes inside the same code, and cmcd_kernels.hip is hashed for the stored counter figures (bench.py:
// kernel_sources_sha).  Folding traj_kernel in is a separate decision.  Until then a change to the network evaluation or the key
// chain is made here AND there; the segment's forward-call test and the reverse parity cases fail when one is forgotten.
//
// What is here is what could move WITHOUT changing a kernel's machine code (tools/probes/device_asm_diff.py, CHANGELOG round 12).
// The LDS staging, q's constants and log q, grad log q with the clips, the z_0 draw, the two ends of a step and the head of the
// statistics record stayed in the two kernels: as helpers each of them compiled to other code (another register allocation over
// the whole kernel, other scratch sizes on the funnel geffner instances), for reasons that have nothing to do with what they
// compute — a helper is simplified on its own before it is inlined, and one that reads blockDim.x no longer folds it to the
// launch's uniform workgroup size.
//
// Mapping: one wave owns 16 particles, lane (g, c) holds particle c and the hidden units {16 t + 4 g + r}; layer 2 on
// v_mfma_f32_16x16x4_f32 with the packed W2 A fragments streamed from LDS, layers 1 and 3 on the VALU from the w1z / w3t tables,
// the per-bridge bias row (and the geffner residual row) from the prep tables.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cmcd_common.h"
#include "cmcd_device.h"
#include "cmcd_hip.h"
#include "cmcd_host.h"

namespace cmcd {

// ------------------------------------------------------------------------------------------
// score network
// ------------------------------------------------------------------------------------------
// the A fragments of input tile ti + 1 requested while tile ti's matrix instructions run: the forward kernel's rule
constexpr bool tile_pf(int ARCH, int D, int T) { return T == 9 || (D == 2 && (T == 2 || ARCH == CMCD_ARCH_DDS)); }

// s(z, idx) for the 16 particles of this wave; brow / urow = row idx of the bias / residual tables (traj_kernel's eval_net).
//   dds     (nn_dds.py:159-162): h1 = gelu(W1^T [z; tau] + b1); h2 = gelu(W2^T h1 + b2); clip(W3^T h2 + b3, +-1e4)
//   geffner (nn.py:45-52,66-70): u = [z; emb]; u += softplus(u W1 + b1); u += softplus(u W2 + b2); factor (u W3 + b3)
// USEL_BY_ROW: how the geffner net writes "the first D entries of u are z" — the same values either way.  The segment kernel uses
// traj_kernel's form (compare every neuron index with every coordinate); the reverse kernel was written with the other (compare
// the lane row), and compiled with traj_kernel's its eight geffner instances come out differently: gmm T = 2 102 VGPRs for 96
// (5 -> 4 waves per SIMD), funnel T = 4 124 bytes of scratch for 116 (CHANGELOG round 12).  So each kernel keeps its form.
template <int ARCH, int D, int T, bool PF, bool USEL_BY_ROW>
__device__ __forceinline__ void tile_eval_net(const float (&z)[D], const float* __restrict__ brow,
                                              const float* __restrict__ urow, const float* lds_w2, const float* lds_w1z,
                                              const float* lds_b2, const float* lds_w3t, const float* lds_b3, int lane,
                                              float (&s)[D]) {
  constexpr int HP = 16 * T;
  const int g = lane >> 4;
  asm volatile("" ::: "memory");  // keep the LDS-resident weights streaming (no LICM into VGPRs)
  f32x4 h[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    f32x4 pre = *reinterpret_cast<const f32x4*>(brow + 16 * t + 4 * g);
#pragma unroll
    for (int j = 0; j < D; ++j) pre += z[j] * *reinterpret_cast<const f32x4*>(lds_w1z + j * HP + 16 * t + 4 * g);
    if (ARCH == CMCD_ARCH_DDS) {
#pragma unroll
      for (int r = 0; r < 4; ++r) h[t][r] = gelu_fast(pre[r]);
    } else {
      f32x4 u = *reinterpret_cast<const f32x4*>(urow + 16 * t + 4 * g);
      if (16 * t < D) {  // the first D neurons of u are z itself
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (USEL_BY_ROW) {
#pragma unroll
            for (int gg = 0; gg < 4; ++gg)   // row gg holds entry 16 t + 4 gg + r
              if (16 * t + 4 * gg + r < D) u[r] = (g == gg) ? z[(16 * t + 4 * gg + r) % D] : u[r];
          } else {   // traj_kernel's form
            const int nidx = 16 * t + 4 * g + r;
#pragma unroll
            for (int j = 0; j < D; ++j)
              if (j >= 16 * t && j < 16 * t + 16) u[r] = (nidx == j) ? z[j] : u[r];
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) h[t][r] = u[r] + softplus(pre[r]);
    }
  }
  // layer 2 on the matrix cores: acc[to] rows = neurons 16 to + 4 g + r, columns = particles
  f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = *reinterpret_cast<const f32x4*>(lds_b2 + 16 * t + 4 * g);
  if (PF) {
    f32x4 af[2][T];
    asm volatile("" ::: "memory");
#pragma unroll
    for (int to = 0; to < T; ++to) af[0][to] = *reinterpret_cast<const f32x4*>(lds_w2 + (to * 64 + lane) * 4);
#pragma unroll
    for (int ti = 0; ti < T; ++ti) {
      asm volatile("" ::: "memory");
      if (ti + 1 < T) {
#pragma unroll
        for (int to = 0; to < T; ++to)
          af[(ti + 1) & 1][to] = *reinterpret_cast<const f32x4*>(lds_w2 + (((ti + 1) * T + to) * 64 + lane) * 4);
      }
      __builtin_amdgcn_sched_barrier(0);   // the reads stay in front of the matrix instructions they overlap
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int to = 0; to < T; ++to)
          acc[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ti & 1][to][r], h[ti][r], acc[to], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
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
  }
  // layer 3: every lane sums over its 4 T neurons, then the 4 lanes of a particle combine
  float part[D];
#pragma unroll
  for (int j = 0; j < D; ++j) part[j] = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    f32x4 h2;
#pragma unroll
    for (int r = 0; r < 4; ++r) h2[r] = (ARCH == CMCD_ARCH_DDS) ? gelu_fast(acc[t][r]) : h[t][r] + softplus(acc[t][r]);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(lds_w3t + j * HP + 16 * t + 4 * g);
      part[j] += h2[0] * wv[0] + h2[1] * wv[1] + h2[2] * wv[2] + h2[3] * wv[3];
    }
  }
  const float factor = lds_b3[15];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float o = group_sum(part[j]) + lds_b3[j];
    s[j] = (ARCH == CMCD_ARCH_DDS) ? fminf(fmaxf(o, -1e4f), 1e4f) : o * factor;
  }
}

// ------------------------------------------------------------------------------------------
// key chain (mcdboundingmachine.py:151-162, mcd_cais.py:66,87,94)
// ------------------------------------------------------------------------------------------
// this lane row's block of split(key): row g computes block gb = g & 1, rows01 of x0 / x1 then hands every lane both halves
__device__ __forceinline__ void tile_split(uint32_t k0, uint32_t k1, int gb, uint32_t& x0, uint32_t& x1) {
  x0 = gb; x1 = 2 + gb;
  threefry2x32(k0, k1, x0, x1);
}

// one step of the key chain: (G, H) = split(gen); nz = normal(G, (D,)); gen = second(split(H)).  Lane row g computes block
// (g & 1) of split(gen); the 2 + ceil(D / 2) blocks of split(H) and normal(G) are dealt to the four rows (traj_kernel's).
template <int D>
__device__ __forceinline__ void tile_chain_step(uint32_t& k0, uint32_t& k1, int g, float (&nz)[2 * ((D + 1) / 2)]) {
  constexpr int Hh = (D + 1) / 2;
  constexpr int NB = 2 + Hh;
  const int gb = g & 1;
  uint32_t x0 = gb, x1 = 2 + gb;
  threefry2x32(k0, k1, x0, x1);
  uint32_t g0, g1, h0, h1;
  rows01(x0, g0, g1);
  rows01(x1, h0, h1);
#pragma unroll
  for (int b0 = 0; b0 < NB; b0 += 4) {
    const int b = b0 + g;
    const bool is_split = b < 2;
    const int jn = b - 2;   // block of normal(G): encrypts (jn, Hh + jn), pad counter 0
    uint32_t y0 = is_split ? b : jn;
    uint32_t y1 = is_split ? 2 + b : ((Hh + jn < D) ? Hh + jn : 0);
    threefry2x32(is_split ? h0 : g0, is_split ? h1 : g1, y0, y1);
    if (b0 == 0) rows01(y1, k0, k1);
    if (D == 2) {
      // the one normal block sits on row 2 with both words: word 1 moves to row 3, one conversion serves both
      uint32_t t0, t1;
      swap16(y1, y1, t0, t1);
      const float dev = bits_to_normal(g == 3 ? t0 : y0);
      uint32_t rr[4];
      rows0123(__float_as_uint(dev), rr);
      nz[0] = __uint_as_float(rr[2]);
      nz[1] = __uint_as_float(rr[3]);
    } else {
      uint32_t r0[4], r1[4];
      rows0123(__float_as_uint(bits_to_normal(y0)), r0);
      rows0123(__float_as_uint(bits_to_normal(y1)), r1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int jj = b0 + q - 2;
        if (jj >= 0 && jj < Hh) {
          nz[jj] = __uint_as_float(r0[q]);
          nz[Hh + jj] = __uint_as_float(r1[q]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// per-wave statistics over lanes 0..15: fixed butterfly order -> deterministic
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void tile_stats_butterfly(double& cnt, double& sm, double& sq, double& mx) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    cnt += __shfl_xor(cnt, o);
    sm += __shfl_xor(sm, o);
    sq += __shfl_xor(sq, o);
    mx = fmax(mx, __shfl_xor(mx, o));
  }
}
__device__ __forceinline__ void tile_stats_butterfly(double& ex) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) ex += __shfl_xor(ex, o);
}

// ------------------------------------------------------------------------------------------
// host: instance table and launch.  Family supplies `fn` and `get<TARGET, ARCH, D, T>()`, the kernel instance.
// ------------------------------------------------------------------------------------------
template <class Family, int TARGET>
static typename Family::fn tile_pick_geffner2(int T) {
  switch (T) {
    case 2: return Family::template get<TARGET, CMCD_ARCH_GEFFNER, 2, 2>();
    case 4: return Family::template get<TARGET, CMCD_ARCH_GEFFNER, 2, 4>();
    case 9: return Family::template get<TARGET, CMCD_ARCH_GEFFNER, 2, 9>();
    default: return nullptr;
  }
}

// the instances of the forward wave-per-tile kernel: gmm / many_gmm (d = 2) and funnel (d = 10); dds 64, geffner on 2, 4
// and 9 neuron tiles (funnel: 4 and 9 — its widths start at 4 tiles, cmcd_api.hip: hidden_width)
template <class Family>
static typename Family::fn tile_pick(const cmcd_desc& d, int T) {
  if (d.mode == CMCD_MODE_CAIS_UHA_SN || d.target == CMCD_TARGET_LGCP) return nullptr;
  if (d.arch == CMCD_ARCH_DDS) {
    if (T != 4) return nullptr;
    if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) return Family::template get<CMCD_TARGET_MANY_GMM, CMCD_ARCH_DDS, 2, 4>();
    if (d.target == CMCD_TARGET_GMM && d.dim == 2) return Family::template get<CMCD_TARGET_GMM, CMCD_ARCH_DDS, 2, 4>();
    if (d.target == CMCD_TARGET_FUNNEL && d.dim == 10) return Family::template get<CMCD_TARGET_FUNNEL, CMCD_ARCH_DDS, 10, 4>();
    return nullptr;
  }
  if (d.arch != CMCD_ARCH_GEFFNER) return nullptr;
  if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) return tile_pick_geffner2<Family, CMCD_TARGET_MANY_GMM>(T);
  if (d.target == CMCD_TARGET_GMM && d.dim == 2) return tile_pick_geffner2<Family, CMCD_TARGET_GMM>(T);
  if (d.target == CMCD_TARGET_FUNNEL && d.dim == 10) {
    if (T == 4) return Family::template get<CMCD_TARGET_FUNNEL, CMCD_ARCH_GEFFNER, 10, 4>();
    if (T == 9) return Family::template get<CMCD_TARGET_FUNNEL, CMCD_ARCH_GEFFNER, 10, 9>();
  }
  return nullptr;
}

template <class Args>
static int tile_launch(void (*fn)(Args), const cmcd_desc& d, const WsLayout& w, const Args& args, hipStream_t stream) {
  const int64_t tiles = w.n_waves, D = d.dim;
  const size_t lds_bytes = size_t(w.HP * w.HP + 2 * D * w.HP + w.HP + 16 + w.tgt_floats) * 4;
  if (lds_bytes > 160 * 1024) return fail(CMCD_ERR_UNSUPPORTED, "network too wide for LDS%s");
  // waves per workgroup: the forward wave-per-tile kernel's rule (cmcd_kernels.hip: traj_launch)
  const int64_t per_cu = (160 * 1024) / (int64_t)lds_bytes;
  int nw = tiles <= 1024 ? 1 : (tiles <= 8192 ? 4 : 8);
  if (per_cu < 2 && tiles > 256) nw = tiles <= 1024 ? 4 : 8;
  CMCD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds_bytes));
  const unsigned blocks = unsigned((tiles + nw - 1) / nw);
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64 * nw), lds_bytes, stream, args);
  return CMCD_OK;
}

}  // namespace cmcd
