// The wave-per-tile pieces that more than one kernel file uses: the score network on 16 particles per wave, the key split, the
// normal(key, (D,)) draw and one step of the key chain, the statistics butterflies and the whole record of a tile, many_gmm's
// constant staging, the two instance tables and the launch.  Each kernel file keeps its chain: direction, what opens and what
// closes a step, how it enters and leaves.
//
// Who includes it and what it takes:
//   cmcd_reverse.hip, cmcd_segment.hip  tile_eval_net, tile_split, tile_chain_step, the two butterflies, tile_pick, tile_launch
//   cmcd_segment_uha.hip  tile_split, tile_normal, tile_chain_step, tile_stats_record (network and launch: its own, below)
//   cmcd_reverse_uha.hip  the same four (network and launch: its own, below)
//   cmcd_reverse_ldvi.hip, cmcd_reverse_hais.hip (through cmcd_mom.h)  the same four; the second also tile_stage_many_gmm, tile_pick_plain
//   cmcd_segment_ldvi.hip, cmcd_segment_hais.hip (through cmcd_mom.h)  what their reverse siblings take
//   cmcd_hais.hip    hais_traj_kernel: tile_split, tile_normal, tile_chain_step, tile_stats_record; both kernels:
//                    tile_stage_many_gmm; tile_pick_plain
//   cmcd_mfvi.hip    tile_pick_plain (mfvi_kernel itself stays on inline copies, below)
//   cmcd_grad.hip    grad_kernel's whole-chain local-gradient instances: tile_normal, tile_chain_step; ula_grad_kernel's table:
//                    tile_pick_plain
//
// The copies that remain, and why.  A change to the network evaluation, the draw or the key chain is made here AND there; the
// segment's forward-call test, the reverse parity cases and tests/test_gpu_hais.py's zero-step-size cases fail when one is
// forgotten.
//   traj_kernel (cmcd_kernels.hip) and coop_kernel (cmcd_coop.hip) hold the first copies, with their debug outputs and ablation
//     probes inside the same code; both files are hashed for the stored counter figures (bench.py: kernel_sources_sha).
//   uha_traj_kernel and uha_coop_kernel (cmcd_uha.hip): its draw_normal carries the capture hooks, the cooperative kernel has a
//     split Threefry of its own, and replacing only the two statistics tails by tile_stats_record changed the body of all 40
//     instances for about 36 lines less.  A separate decision.
//   segment_uha_kernel (cmcd_segment_uha.hip) and the LDVI kernels (cmcd_ldvi.hip) each hold a copy of cmcd_uha.hip's
//     net_pre_z / net_eval_rho (the network on [z; rho]): that file is hashed, so the two functions cannot move here.  The segment
//     kernel also has a launch of its own (W1 has 2 D input rows: one more D * HP block of LDS than tile_launch sizes for) and an
//     instance table of its own (uha_pick's: geffner on 5 neuron tiles as well); tests/test_gpu_smc_uha.py's forward-call test
//     fails when its copy drifts.
//   reverse_uha_kernel (cmcd_reverse_uha.hip) holds the third copy of the pair, as rev_pre_z / rev_eval_rho (copied from
//     seg_pre_z / seg_eval_rho), with a launch and an instance table that repeat segment_uha_launch's and segment_uha_pick's;
//     tests/test_gpu_reverse_uha.py's parity cases (all five widths and dds) fail when its copy drifts.
//   reverse_ldvi_kernel (cmcd_reverse_ldvi.hip) takes the pair's geffner branch from cmcd_mom.h (mom_pre_z / mom_eval_rho, copied from
//     ldvi_pre_z / ldvi_eval_rho: cmcd_ldvi.hip stays as it is), the header it shares with reverse_hais_kernel
//     (cmcd_reverse_hais.hip), whose beta table is a copy of cmcd_hais.hip's hais_form_betas; tests/test_gpu_reverse_ldvi.py's and
//     tests/test_gpu_reverse_hais.py's parity cases fail when those copies drift.  segment_ldvi_kernel (cmcd_segment_ldvi.hip) and
//     segment_hais_kernel (cmcd_segment_hais.hip) take the same header: no further copy.
//   reverse_traj_kernel and segment_traj_kernel keep inline the LDS staging, q's constants and log q, grad log q with the clips,
//     the z_0 draw, the two ends of a step and the head of the statistics record: as helpers each of them compiled to other code
//     (another register allocation over the whole kernel, other scratch sizes on the funnel geffner instances), for reasons that
//     have nothing to do with what they compute — a helper is simplified on its own before it is inlined, and one that reads
//     blockDim.x no longer folds it to the launch's uniform workgroup size.  Their device code is byte-identical to the build
//     before the header existed (tools/probes/device_asm_diff.py, CHANGELOG round 12) and stays so.
//   grad_kernel's prologue splits (cmcd_grad.hip) and ula_grad_kernel were not touched.
//   mfvi_kernel (cmcd_mfvi.hip) keeps its staging, split, draw and statistics record inline: on tile_stage_many_gmm, tile_split,
//     tile_normal and tile_stats_record it kept its registers (39 / 55 / 58 VGPRs, no scratch, 8 waves per SIMD) and its bits, but
//     the mean-field gradient call on many_gmm with 15 000 particles went from 52.6 us to 53.7 / 55.0 us in two processes against
//     a spread of 0.3 us over the previous build's windows (profiles/r14_tile_plain_ab.txt, section 5).
// The network-free kernels do not keep their bytes on the helpers (hais_traj_kernel and the ten whole-chain local-gradient
// instances of grad_kernel compile to other code; hais_grad_kernel does not).  Their bar: no more scratch, no occupancy step lost,
// bit-identical results, the previous build's timing spread (CHANGELOG round 16, profiles/r14_tile_plain_device_asm.txt,
// profiles/r14_tile_plain_ab.txt); a kernel that misses it keeps its inline copy and is named here with the numbers.
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

// normal(key, (D,)): block j encrypts (j, Hh + j), pad counter 0; the blocks are dealt to the four rows of the wave
template <int D>
__device__ __forceinline__ void tile_normal(uint32_t ka, uint32_t kb, int g, float (&nz)[2 * ((D + 1) / 2)]) {
  constexpr int Hh = (D + 1) / 2;
#pragma unroll
  for (int j0 = 0; j0 < Hh; j0 += 4) {
    const int j = j0 + g;
    uint32_t y0 = j, y1 = (Hh + j < D) ? Hh + j : 0;
    threefry2x32(ka, kb, y0, y1);
    uint32_t r0[4], r1[4];
    rows0123(__float_as_uint(bits_to_normal(y0)), r0);
    rows0123(__float_as_uint(bits_to_normal(y1)), r1);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (j0 + q < Hh) {
        nz[j0 + q] = __uint_as_float(r0[q]);
        nz[Hh + j0 + q] = __uint_as_float(r1[q]);
      }
  }
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

// the whole record of a tile over l := loss: {finite count, sum, sum of squares, max of -l, sum exp(-l - max)} -> out5, by lane 0.
// `use`: this lane holds a particle of the batch and is the one of its four lanes that counts (lane row 0).
__device__ __forceinline__ void tile_stats_record(float loss, bool use, int lane, double* out5) {
  double cnt = (use && isfinite(loss)) ? 1.0 : 0.0;
  double sm = use ? (double)loss : 0.0;
  double sq = use ? (double)loss * (double)loss : 0.0;
  double mx = use ? -(double)loss : -INFINITY;
  tile_stats_butterfly(cnt, sm, sq, mx);
  double ex = (use && mx > -INFINITY && mx < INFINITY) ? exp(-(double)loss - mx) : 0.0;
  tile_stats_butterfly(ex);
  if (lane == 0) {
    out5[0] = cnt; out5[1] = sm; out5[2] = sq; out5[3] = mx; out5[4] = ex;
  }
}

// ------------------------------------------------------------------------------------------
// many_gmm's constants as Target<>::eval expects them in LDS, by the whole workgroup: {scale, means} as handed to the C ABI ->
// {1/scale, c2, n_mix bits, c0, means} (log2 units).  The caller keeps its `if (TARGET == CMCD_TARGET_MANY_GMM)` and its barrier.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void tile_stage_many_gmm(const float* tc, int n_mix, float* lds_tgt) {
  const float s = tc[0];
  for (int idx = threadIdx.x; idx < 4 + 2 * n_mix; idx += blockDim.x) {
    float v;
    if (idx == 0) v = 1.0f / s;
    else if (idx == 1) v = -0.5f * 1.44269504088896340736f / (s * s);
    else if (idx == 2) v = __int_as_float(n_mix);
    else if (idx == 3) v = 1.44269504088896340736f * (-2.0f * (logf(s) + kHalfLog2Pi) - logf((float)n_mix));
    else v = tc[1 + (idx - 4)];
    lds_tgt[idx] = v;
  }
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

// the instances of the network-free wave-per-tile kernels (mean-field, Hamiltonian AIS, MCD_ULA's sweep): the same three
// (target, dim) pairs.  Family supplies `fn` and `get<TARGET, D>()`.
template <class Family>
static typename Family::fn tile_pick_plain(int target, int dim) {
  if (target == CMCD_TARGET_GMM && dim == 2) return Family::template get<CMCD_TARGET_GMM, 2>();
  if (target == CMCD_TARGET_MANY_GMM && dim == 2) return Family::template get<CMCD_TARGET_MANY_GMM, 2>();
  if (target == CMCD_TARGET_FUNNEL && dim == 10) return Family::template get<CMCD_TARGET_FUNNEL, 10>();
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
