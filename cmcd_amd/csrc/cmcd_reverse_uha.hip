// The reverse-time chain of 2nd-order (underdamped) CMCD, MCD_CAIS_UHA_sn, on gfx950: target draws pushed through the BACKWARD
// kernels of the sampler, the momentum refreshed by B_i and the leap-frog of every bridge inverted — the call cmcd_reverse.hip
// has no kernel for.
//
// The reference has no such call; what is restated here is the arithmetic of its forward chain (cmcd_uha.hip: uha_traj_kernel,
// reference lines mcd_under_lp_a_cais.py:41-113, mcdboundingmachine.py:126-179), walked the other way, and is written out in
// include/cmcd_hip.h (cmcd_bound_reverse_uha).  Per particle, with the schedules beta_i, eps_i (cos^2), the clip of grad log p at
// 1e2, gamma, the network s([z; rho], i) and q of cmcd_bound_forward in this mode (the same prep tables), eta_i = gamma eps_i,
// sigma_i = sqrt(2 eta_i), gU(z, b) = -(b clip(grad log p(z)) + (1 - b) grad log q(z)):
//
//   z_K = x;  rho_K = normal(R);  w = log p(z_K) + log N(rho_K; 0, I)
//   for i = K-1 .. 0:
//     rho'' = rho_{i+1} + eps_i gU(z_{i+1}, beta_i) / 2                               :65-67 undone (the second half-kick)
//     z_i   = z_{i+1} - eps_i rho''                                                   :63 undone    (the drift)
//     rho'  = rho'' + eps_i gU(z_i, beta_i) / 2                                       :62 undone    (the first half-kick)
//     m_b   = rho' (1 - eta_i) + 2 eta_i s([z_i; rho'], i)                            :77-80        (z_i, the SAME index i)
//     rho_i = m_b + sigma_i xi_r,  r = K-1-i                                          (the draw the forward chain takes from F_i)
//     m_f   = rho_i (1 - eta_i) - 2 eta_i s([z_i; rho_i], i)                          :52-54
//     w    += log N(rho_i; m_b, sigma_i) - log N(rho'; m_f, sigma_i)                  :83-88
//   w -= log q(z_0) + log N(rho_0; 0, I)
//
// i.e. the functional the forward call returns as -loss, on a path drawn from p(z_K) N(rho_K) prod B_i: E[w] >= ln Z (the EUBO),
// and exp(-w) are the importance weights of the reverse estimate of 1 / Z.  The leap-frog is a volume-preserving bijection: no
// Jacobian term.  The densities sit at the z_i the inverted leap-frog produces; whether a float32 forward leap-frog from
// (z_i, rho') lands on (z_{i+1}, rho_{i+1}) again does not enter w.
//
// Key chain = the forward call's for this mode (mcdboundingmachine.py:151-162; mcd_under_lp_a_cais.py:92-93,100) without its first
// draw: (_, B) = split(PRNGKey(seed)); C = first(split(B)); (R, G') = split(C); rho_K = normal(R) (the key the forward chain spends
// on rho_0); gen_0 = second(split(G')); reverse step r: (G, H) = split(gen), xi_r = normal(G, (d,)), gen = second(split(H)).
//
// ONE rotated loop, m = K .. 0, with a SINGLE site that evaluates (log p, grad log p, grad log q) at z_m.  For m < K that
// evaluation closes the inverse leap-frog of bridge m (rho' = rho'' + eps_m uf / 2); the two network evaluations — both at z_m,
// both with row m, so the z part of the first layer is formed once — and both densities of bridge m follow.  For m > 0 it opens
// bridge m - 1 (rho'', then z_{m-1}) with row m - 1 of the schedule; at m == K it gives log p(z_K).  K + 1 target evaluations and
// 2 K network evaluations: the forward kernel's count.
//
// Mapping = uha_traj_kernel's and segment_uha_kernel's: one wave owns 16 particles for all K steps, lane (g, c) holds particle c
// and the hidden units {16 t + 4 g + r}; layer 2 on v_mfma_f32_16x16x4_f32 with the packed W2 A fragments streamed from LDS,
// layers 1 and 3 on the VALU; z, rho, w and the key stay in registers; one statistics record per tile over l := w for
// finalize_kernel.  rev_pre_z / rev_eval_rho are COPIES of cmcd_uha.hip's net_pre_z / net_eval_rho, as cmcd_segment_uha.hip's and
// cmcd_ldvi.hip's are: that file is hashed for the stored counter figures (bench.py: kernel_sources_sha) and cannot hand them
// out through a header.  The key-chain step, the draw, the split and the statistics record are cmcd_tile.h's.  Plain vector
// stores only.  A particle whose x row holds a non-finite entry, or whose w comes out NaN, leaves with w = +inf (weight 0).
#include "cmcd_tile.h"

namespace cmcd {

struct ReverseUhaArgs {
  TrajArgs t;       // seeds, params, ws, partials, lay, w, n, K; out_loss = out_w, out_z = out_z0; the rest unused
  const float* x;   // [n][D] target draws
  float* rho0;      // [n][D] out: the momentum at the q end
};

// first-layer pre-activation shared by the two evaluations of a bridge: bias row (time path folded by the prep launch) + z W1[:d]
// (cmcd_uha.hip: net_pre_z)
template <int D, int T>
__device__ __forceinline__ void rev_pre_z(const float (&z)[D], const float* __restrict__ brow, const float* lds_w1z, int g,
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

// s([z; rho], i) for the 16 particles of this wave, given the shared part of the first layer (cmcd_uha.hip: net_eval_rho)
//   dds     (nn_dds.py:159-162): h1 = gelu(W1^T [z; rho; tau] + b1); h2 = gelu(W2^T h1 + b2); clip(W3^T h2 + b3, +-1e4)
//   geffner (nn.py:45-52,66-70): u = [z; rho; emb]; u += softplus(u W1 + b1); u += softplus(u W2 + b2); factor (u W3 + b3)
template <int ARCH, int D, int T>
__device__ __forceinline__ void rev_eval_rho(const f32x4 (&prez)[T], const float (&z)[D], const float (&rho)[D],
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
    if (ARCH == CMCD_ARCH_DDS) {
#pragma unroll
      for (int r = 0; r < 4; ++r) h[t][r] = gelu_fast(pre[r]);
    } else {
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

// a value every lane of the wave holds alike (a parameter, a schedule entry), moved to a scalar register: the loads below are
// vector loads (params and ws are not known to be unwritten), and D = 10 leaves the geffner instances no vector register to
// spare for 2 D + 3 loop-invariant copies
__device__ __forceinline__ float rev_uniform(float v) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

template <int TARGET, int ARCH, int D, int T>
__global__ __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4) void reverse_uha_kernel(ReverseUhaArgs ra) {
  const TrajArgs& a = ra.t;
  constexpr int HP = 16 * T;
  constexpr int Hh = (D + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lds_w2 = lds;                     // HP*HP
  float* lds_w1z = lds_w2 + HP * HP;       // 2D*HP   rows [0, D) = z part, [D, 2D) = rho part
  float* lds_w3t = lds_w1z + 2 * D * HP;   // D*HP
  float* lds_b2 = lds_w3t + D * HP;        // HP
  float* lds_b3 = lds_b2 + HP;             // 16
  float* lds_tgt = lds_b3 + 16;            // tgt_floats
  const int K = a.K;
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(a.ws + a.w.w1z);
    f32x4* dst = reinterpret_cast<f32x4*>(lds_w1z);
    for (int i = threadIdx.x; i < 2 * D * HP / 4; i += blockDim.x) dst[i] = src[i];
    src = reinterpret_cast<const f32x4*>(a.ws + a.w.w2);
    dst = reinterpret_cast<f32x4*>(lds_w2);
    for (int i = threadIdx.x; i < HP * HP / 4; i += blockDim.x) dst[i] = src[i];
    src = reinterpret_cast<const f32x4*>(a.ws + a.w.w3t);
    dst = reinterpret_cast<f32x4*>(lds_w3t);
    for (int i = threadIdx.x; i < D * HP / 4; i += blockDim.x) dst[i] = src[i];
    for (int i = threadIdx.x; i < HP; i += blockDim.x) lds_b2[i] = a.ws[a.w.b2 + i];
    for (int i = threadIdx.x; i < 16; i += blockDim.x) lds_b3[i] = a.ws[a.w.b3 + i];
    for (int i = threadIdx.x; i < a.w.tgt_floats; i += blockDim.x) lds_tgt[i] = a.ws[a.w.tgt + i];
    // the per-bridge tables into this XCD's L2, one touch per 128-byte line (as the forward kernel does)
    float warm = 0.f;
    const int64_t t0 = a.w.sched;
    const int64_t t1 = (ARCH == CMCD_ARCH_GEFFNER ? a.w.utab : a.w.bias1) + (int64_t)(K + 1) * HP;
    const int64_t per_xcd = (gridDim.x + 7) >> 3, rank = blockIdx.x >> 3;
    for (int64_t i = t0 + 32 * (rank * blockDim.x + threadIdx.x); i < t1; i += 32 * per_xcd * blockDim.x) warm += a.ws[i];
    asm volatile("" ::"v"(warm));
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wave * 16 >= a.n) return;  // whole wave out of range (after the only barrier)
  const int64_t p = wave * 16 + c;
  const bool valid = p < a.n;
  const int64_t pl = valid ? p : a.n - 1;   // the lanes past the batch repeat its last particle and store nothing

  // q = N(mean, exp(logdiag)^2)
  float qmean[D], qiv[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    qmean[j] = rev_uniform(a.params[a.lay.vd_mean + j]);
    const float qstd = expf(a.params[a.lay.vd_logdiag + j]);
    qiv[j] = rev_uniform(1.0f / (qstd * qstd));
  }
  const float gamma = rev_uniform(a.params[a.lay.gamma]);

  // z_K = x
  float z[D], rho[D];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    z[j] = ra.x[pl * D + j];
    bad = bad || !isfinite(z[j]);
  }

  // ---- key chain: (_, B) = split(PRNGKey(seed)); C = first(split(B)); (R, G') = split(C); rho_K = normal(R);
  // gen_0 = second(split(G'))
  const int gb = g & 1;
  uint32_t k0, k1;
  {
    const int32_t seed = a.seeds[pl];
    uint32_t x0, x1;
    tile_split(0u, (uint32_t)seed, gb, x0, x1);   // (A, B); A (the forward call's z_0 key) is not used
    uint32_t b0, b1;
    rows01(x1, b0, b1);
    tile_split(b0, b1, gb, x0, x1);
    uint32_t c0, c1;
    rows01(x0, c0, c1);
    tile_split(c0, c1, gb, x0, x1);
    uint32_t r0, r1, p0, p1;
    rows01(x0, r0, r1);
    rows01(x1, p0, p1);
    float nz[2 * Hh];
    tile_normal<D>(r0, r1, g, nz);
#pragma unroll
    for (int j = 0; j < D; ++j) rho[j] = nz[j];
    tile_split(p0, p1, gb, x0, x1);
    rows01(x1, k0, k1);
  }

  const float* bias1 = a.ws + a.w.bias1;
  const float* utab = a.ws + a.w.utab;
  constexpr float clipv = 1e2f;   // gradU(z, beta, clip=1e2), stable=True      mcd_under_lp_a_cais.py:23-30,42,46

  // Rotated loop over the states z_K .. z_0: iteration m evaluates log p, grad log p and grad log q ONCE, at z_m.
  // `rho` holds rho_K on entry, rho'' of bridge m at the top of every later iteration, and rho_m once the bridge is closed.
  float pbeta = 0.f, peps = 0.f;     // schedule row m (set when bridge m was opened)
  float w = 0.f;                     // log N(rho_K; 0, I); log p(z_K) joins it at m == K
#pragma unroll
  for (int j = 0; j < D; ++j) w += -(rho[j] * rho[j]) * 0.5f - kHalfLog2Pi;

  for (int m = K; m >= 0; --m) {
    float gp[D], gq[D], logp;
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      gp[j] = fminf(fmaxf(gp[j], -clipv), clipv);
      gq[j] = -(z[j] - qmean[j]) * qiv[j];
    }

    // the half-kick that opens bridge m - 1, eps_{m-1} gU(z_m, beta_{m-1}) / 2, formed here so that grad log p and grad log q
    // are not carried over the network evaluations (m == 0: row 0 again, unused)
    const int mo = m > 0 ? m - 1 : 0;
    const float beta = rev_uniform(a.ws[a.w.beta + mo]), eps = rev_uniform(a.ws[a.w.eps + mo]);
    float hk[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float ub = -1.0f * (beta * gp[j] + (1.0f - beta) * gq[j]);     // :65 (beta_{m-1})
      hk[j] = eps * ub / 2.0f;
    }

    if (m == K) {
      w = logp + w;   // w = log p(z_K) + log N(rho_K; 0, I)
    } else {
      // ---- bridge m: the first half-kick undone at z_m, then the backward draw of the momentum and both kernels' densities
      const float eta = gamma * peps;                   // :50
      const float sig = sqrtf(2.0f * eta);              // :56
      const float inv2s2 = 1.0f / (2.0f * sig * sig), cst = logf(sig) + kHalfLog2Pi;
      const float ome = 1.0f - eta;
      float rhop[D];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float uf = -1.0f * (pbeta * gp[j] + (1.0f - pbeta) * gq[j]);
        rhop[j] = rho[j] + peps * uf / 2.0f;                          // :62 undone
      }
      f32x4 prez[T];
      rev_pre_z<D, T>(z, bias1 + (int64_t)m * HP, lds_w1z, g, prez);
      float s1[D], s2[D];
      rev_eval_rho<ARCH, D, T>(prez, z, rhop, utab + (int64_t)m * HP, lds_w2, lds_w1z, lds_b2, lds_w3t, lds_b3, lane, s2);
      float nz[2 * Hh];
      tile_chain_step<D>(k0, k1, g, nz);                // (G, H) = split(gen); xi_r = normal(G); gen = second(split(H))
      float bk_lp = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float mb = rhop[j] * ome + 2.0f * eta * s2[j];          // :77-80
        rho[j] = mb + sig * nz[j];
        const float db = rho[j] - mb;
        bk_lp += -(db * db) * inv2s2 - cst;                           // log N(rho_m; m_b, sigma)   :84
      }
      rev_eval_rho<ARCH, D, T>(prez, z, rho, utab + (int64_t)m * HP, lds_w2, lds_w1z, lds_b2, lds_w3t, lds_b3, lane, s1);
      float fk_lp = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float mf = rho[j] * ome - 2.0f * eta * s1[j];           // :52-54
        const float df = rhop[j] - mf;
        fk_lp += -(df * df) * inv2s2 - cst;                           // log N(rho'; m_f, sigma)    :83
      }
      w += bk_lp - fk_lp;                                             // :88
    }
    if (m == 0) break;

    // ---- bridge m - 1 opened at z_m: the second half-kick and the drift undone
#pragma unroll
    for (int j = 0; j < D; ++j) {
      rho[j] = rho[j] + hk[j];                                             // :67 undone: rho'' of bridge m - 1
      z[j] = z[j] - eps * rho[j];                                          // :63 undone
    }
    pbeta = beta; peps = eps;
  }

  // w -= log q(z_0) + log N(rho_0; 0, I).  q's standard deviations are formed again from the parameters: carried over the loop
  // they would sit in D registers that no bridge reads (the funnel geffner instances have none to spare)
#pragma unroll
  for (int j = 0; j < D; ++j) {
    float ld = a.params[a.lay.vd_logdiag + j];
    asm volatile("" : "+v"(ld));
    const float sd = expf(ld);
    const float dz = z[j] - qmean[j];
    w -= -(dz * dz) / (2.0f * sd * sd) - logf(sd) - kHalfLog2Pi;
  }
  {
    float l0 = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) l0 += -(rho[j] * rho[j]) * 0.5f - kHalfLog2Pi;
    w -= l0;
  }
  if (bad || w != w) w = INFINITY;   // weight exp(-w) = 0, like a diverged particle's loss of the forward call

  if (valid && g == 0) {
    a.out_loss[p] = w;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      a.out_z[p * D + j] = z[j];
      ra.rho0[p * D + j] = rho[j];
    }
  }

  tile_stats_record(w, valid && g == 0, lane, a.partials + wave * CMCD_NSTATS);
}

// ------------------------------------------------------------------------------------------
// launcher (cmcd_host.h): the instances of the forward call's wave-per-tile 2nd-order kernel (cmcd_uha.hip: uha_pick)
// ------------------------------------------------------------------------------------------
typedef void (*reverse_uha_fn)(ReverseUhaArgs);

template <int TARGET, int ARCH, int D>
static reverse_uha_fn reverse_uha_pick_T(int T) {
  switch (T) {
    case 2: return reverse_uha_kernel<TARGET, ARCH, D, 2>;
    case 4: return reverse_uha_kernel<TARGET, ARCH, D, 4>;
    case 5: return reverse_uha_kernel<TARGET, ARCH, D, 5>;
    case 9: return reverse_uha_kernel<TARGET, ARCH, D, 9>;
    default: return nullptr;
  }
}

static reverse_uha_fn reverse_uha_pick(const cmcd_desc& d, int T) {
  if (d.mode != CMCD_MODE_CAIS_UHA_SN) return nullptr;
  if (d.arch == CMCD_ARCH_DDS) {
    if (T != 4) return nullptr;
    if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) return reverse_uha_kernel<CMCD_TARGET_MANY_GMM, CMCD_ARCH_DDS, 2, 4>;
    if (d.target == CMCD_TARGET_GMM && d.dim == 2) return reverse_uha_kernel<CMCD_TARGET_GMM, CMCD_ARCH_DDS, 2, 4>;
    if (d.target == CMCD_TARGET_FUNNEL && d.dim == 10) return reverse_uha_kernel<CMCD_TARGET_FUNNEL, CMCD_ARCH_DDS, 10, 4>;
    return nullptr;
  }
  if (d.arch != CMCD_ARCH_GEFFNER) return nullptr;
  if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) return reverse_uha_pick_T<CMCD_TARGET_MANY_GMM, CMCD_ARCH_GEFFNER, 2>(T);
  if (d.target == CMCD_TARGET_GMM && d.dim == 2) return reverse_uha_pick_T<CMCD_TARGET_GMM, CMCD_ARCH_GEFFNER, 2>(T);
  if (d.target == CMCD_TARGET_FUNNEL && d.dim == 10) return reverse_uha_pick_T<CMCD_TARGET_FUNNEL, CMCD_ARCH_GEFFNER, 10>(T);
  return nullptr;
}

bool reverse_uha_available(const cmcd_desc& d, int T) { return reverse_uha_pick(d, T) != nullptr; }

int reverse_uha_launch(const cmcd_desc& d, const WsLayout& w, const TrajArgs& ta, const float* x, float* rho0,
                       hipStream_t stream) {
  reverse_uha_fn fn = reverse_uha_pick(d, w.T);
  if (!fn) return fail(CMCD_ERR_UNSUPPORTED, "no 2nd-order reverse-chain kernel instance for this (mode, target, dim, arch, width=%s%lld)", "", w.HP);
  const int64_t tiles = w.n_waves, D = d.dim;
  // W1 has 2 D input rows ([z; rho]): one more D * HP block than tile_launch sizes for (segment_uha_launch's size)
  const size_t lds_bytes = size_t(w.HP * w.HP + 3 * D * w.HP + w.HP + 16 + w.tgt_floats) * 4;
  if (lds_bytes > 160 * 1024) return fail(CMCD_ERR_UNSUPPORTED, "network too wide for LDS%s");
  // waves per workgroup: tile_launch's rule (= the forward wave-per-tile kernels')
  const int64_t per_cu = (160 * 1024) / (int64_t)lds_bytes;
  int nw = tiles <= 1024 ? 1 : (tiles <= 8192 ? 4 : 8);
  if (per_cu < 2 && tiles > 256) nw = tiles <= 1024 ? 4 : 8;
  CMCD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds_bytes));
  const unsigned blocks = unsigned((tiles + nw - 1) / nw);
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64 * nw), lds_bytes, stream, ReverseUhaArgs{ta, x, rho0});
  return CMCD_OK;
}

}  // namespace cmcd
