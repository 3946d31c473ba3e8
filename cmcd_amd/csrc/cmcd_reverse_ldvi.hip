// The reverse-time chain of LDVI (MCD_U_a-lp-sn and its network-free sibling MCD_U_a-lp) on gfx950: target draws pushed through
// the BACKWARD kernels of the sampler, the leap-frog of every bridge inverted — the 2nd-order chain of cmcd_reverse_uha.hip with
// three differences: the forward kernel has no network, the step size is the scalar leaf (no cos^2 table), grad log p is not
// clipped.  One network evaluation per bridge, not two.
//
// The reference has no such call; what is restated here is the arithmetic of its forward chain (cmcd_ldvi.hip: ldvi_traj_kernel,
// reference lines mcd_under_lp_a.py:6-87), walked the other way, and is written out in include/cmcd_hip.h
// (cmcd_bound_reverse_ldvi).  Per particle, with eta = gamma eps, sigma = sqrt(2 eta), gU(z, b) = -(b grad log p(z) +
// (1 - b) grad log q(z)) (no clip), eps constant over the bridges (the tree's eta leaf is not read):
//
//   z_K = x;  rho_K = normal(R);  w = log p(z_K) + log N(rho_K; 0, I)
//   for i = K-1 .. 0:
//     rho'' = rho_{i+1} + eps gU(z_{i+1}, beta_i) / 2                          :37 undone (the closing half-kick)
//     z_i   = z_{i+1} - eps rho''                                              :36 undone (the drift)
//     rho'  = rho'' + eps gU(z_i, beta_i) / 2                                  :35 undone (the opening half-kick)
//     m_b   = rho' (1 - eta) [+ 2 eta s([z_i; rho'], i)]                       :41-51     (the network only when NET)
//     rho_i = m_b + sigma xi_r,  r = K-1-i                                     (the draw the forward chain takes from F_i)
//     m_f   = rho_i (1 - eta)                                                  :29
//     w    += log N(rho_i; m_b, sigma) - log N(rho'; m_f, sigma)               :54-58
//   w -= log q(z_0) + log N(rho_0; 0, I)
//
// i.e. the functional the forward call returns as -loss, on a path drawn from p(z_K) N(rho_K) prod B_i: E[w] >= ln Z (the EUBO).
// Key chain = the 2nd-order reverse chain's (cmcd_reverse_uha.hip): the forward chain's without its first draw.
//
// ONE rotated loop, m = K .. 0, with a SINGLE site that evaluates (log p, grad log p, grad log q) at z_m: for m < K it closes the
// inverse leap-frog of bridge m, the network evaluation (row m) and both densities follow; for m > 0 it opens bridge m - 1 with
// beta_{m-1}; at m == K it gives log p(z_K).  K + 1 target evaluations and K network evaluations: the forward kernel's count.
//
// Mapping = ldvi_traj_kernel's (cmcd_tile.h): one wave per 16-particle tile, lane (g, c) = particle c; layer 2 on
// v_mfma_f32_16x16x4_f32 from the packed W2 fragments in LDS (cmcd_mom.h); z, rho, w and the key in registers; one statistics
// record per tile over l := w for finalize_kernel.  Plain vector stores only.  A particle whose x row holds a non-finite entry,
// whose log p(x) is floored (many_gmm) or whose w comes out NaN leaves with w = +inf (weight 0).
#include "cmcd_mom.h"

namespace cmcd {

struct ReverseLdviArgs {
  const int32_t* seeds;
  const float* x;           // [n][D] target draws
  const float* params;
  const float* ws;          // the prep launch's tables
  double* partials;         // [tiles][5]
  float* out_w;
  float* out_z0;
  float* out_rho0;
  cmcd_layout lay;
  WsLayout w;
  int64_t n;
  int32_t K;
};

// Dynamic LDS, ldvi_traj_kernel's: NET: w2 | w1z[2 D] | w3t | b2 | b3[16] | target constants; without a network the constants alone.
template <int TARGET, int D, int T, bool NET>
__global__ __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4) void reverse_ldvi_kernel(ReverseLdviArgs a) {
  constexpr int HP = 16 * T;
  constexpr int Hh = (D + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lds_w2 = lds;                                   // HP*HP
  float* lds_w1z = lds_w2 + (NET ? HP * HP : 0);         // 2D*HP   rows [0, D) = z part, [D, 2D) = rho part
  float* lds_w3t = lds_w1z + (NET ? 2 * D * HP : 0);     // D*HP
  float* lds_b2 = lds_w3t + (NET ? D * HP : 0);          // HP
  float* lds_b3 = lds_b2 + (NET ? HP : 0);               // 16
  float* lds_tgt = lds_b3 + (NET ? 16 : 0);              // tgt_floats
  if (NET) {
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
  }
  for (int i = threadIdx.x; i < a.w.tgt_floats; i += blockDim.x) lds_tgt[i] = a.ws[a.w.tgt + i];
  __syncthreads();

  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (tile * 16 >= a.n) return;  // whole wave out of range (after the only barrier)
  const int64_t p = tile * 16 + c;
  const bool valid = p < a.n;
  const int64_t pl = valid ? p : a.n - 1;   // the lanes past the batch repeat its last particle and store nothing
  const int K = a.K;

  // q = N(mean, exp(logdiag)^2); the constants of every bridge
  float qmean[D], qiv[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    qmean[j] = mom_uniform(a.params[a.lay.vd_mean + j]);
    const float qstd = expf(a.params[a.lay.vd_logdiag + j]);
    qiv[j] = mom_uniform(1.0f / (qstd * qstd));
  }
  const float eps = mom_uniform(a.params[a.lay.eps]), gamma = mom_uniform(a.params[a.lay.gamma]);
  const float eta = gamma * eps;                       // :28
  const float sig = sqrtf(2.0f * eta);                 // :30
  const float inv2s2 = 1.0f / (2.0f * sig * sig), cst = logf(sig) + kHalfLog2Pi;
  const float ome = 1.0f - eta;

  // z_K = x
  float z[D], rho[D];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    z[j] = a.x[pl * D + j];
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

  // Rotated loop over the states z_K .. z_0: iteration m evaluates log p, grad log p and grad log q ONCE, at z_m.
  // `rho` holds rho_K on entry, rho'' of bridge m at the top of every later iteration, and rho_m once the bridge is closed.
  float pbeta = 0.f;                 // beta_m (set when bridge m was opened)
  float w = mom_log_n01<D>(rho);     // log N(rho_K; 0, I); log p(z_K) joins it at m == K

  for (int m = K; m >= 0; --m) {
    float gp[D], gq[D], logp;
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
#pragma unroll
    for (int j = 0; j < D; ++j) gq[j] = -(z[j] - qmean[j]) * qiv[j];

    // the half-kick that opens bridge m - 1, eps gU(z_m, beta_{m-1}) / 2, formed here so that grad log p and grad log q are not
    // carried over the network evaluation (m == 0: row 0 again, unused)
    const int mo = m > 0 ? m - 1 : 0;
    const float beta = mom_uniform(a.ws[a.w.beta + mo]);
    float hk[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float ub = -1.0f * (beta * gp[j] + (1.0f - beta) * gq[j]);     // :37 (beta_{m-1})
      hk[j] = eps * ub / 2.0f;
    }

    if (m == K) {
      w = logp + w;   // w = log p(z_K) + log N(rho_K; 0, I)
      bad = bad || logp == -INFINITY;   // many_gmm: x under the floor of log p
    } else {
      // ---- bridge m: the opening half-kick undone at z_m, then the backward draw of the momentum and both kernels' densities
      float rhop[D], s[D];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float uf = -1.0f * (pbeta * gp[j] + (1.0f - pbeta) * gq[j]);
        rhop[j] = rho[j] + eps * uf / 2.0f;                               // :35 undone
        s[j] = 0.f;
      }
      if (NET) {
        f32x4 prez[T];
        mom_pre_z<D, T>(z, bias1 + (int64_t)m * HP, lds_w1z, g, prez);
        mom_eval_rho<D, T>(prez, z, rhop, utab + (int64_t)m * HP, lds_w2, lds_w1z, lds_b2, lds_w3t, lds_b3, lane, s);
      }
      float nz[2 * Hh];
      tile_chain_step<D>(k0, k1, g, nz);                // (G, H) = split(gen); xi_r = normal(G); gen = second(split(H))
      float bk_lp = 0.f, fk_lp = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float mb = NET ? rhop[j] * ome + 2.0f * eta * s[j] : rhop[j] * ome;   // :41-51
        rho[j] = mb + sig * nz[j];
        const float db = rho[j] - mb;
        bk_lp += -(db * db) * inv2s2 - cst;                               // log N(rho_m; m_b, sigma)   :55
        const float mf = rho[j] * ome;                                    // :29
        const float df = rhop[j] - mf;
        fk_lp += -(df * df) * inv2s2 - cst;                               // log N(rho'; m_f, sigma)    :54
      }
      w += bk_lp - fk_lp;                                                 // :58
    }
    if (m == 0) break;

    // ---- bridge m - 1 opened at z_m: the closing half-kick and the drift undone
#pragma unroll
    for (int j = 0; j < D; ++j) {
      rho[j] = rho[j] + hk[j];                                            // :37 undone: rho'' of bridge m - 1
      z[j] = z[j] - eps * rho[j];                                         // :36 undone
    }
    pbeta = beta;
  }

  // w -= log q(z_0) + log N(rho_0; 0, I).  q's standard deviations are formed again from the parameters: carried over the loop
  // they would sit in D registers that no bridge reads
#pragma unroll
  for (int j = 0; j < D; ++j) {
    float ld = a.params[a.lay.vd_logdiag + j];
    asm volatile("" : "+v"(ld));
    const float sd = expf(ld);
    const float dz = z[j] - qmean[j];
    w -= -(dz * dz) / (2.0f * sd * sd) - logf(sd) - kHalfLog2Pi;
  }
  w -= mom_log_n01<D>(rho);
  if (bad || w != w) w = INFINITY;   // weight exp(-w) = 0, like a diverged particle's loss of the forward call

  if (valid && g == 0) {
    a.out_w[p] = w;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      a.out_z0[p * D + j] = z[j];
      a.out_rho0[p * D + j] = rho[j];
    }
  }

  tile_stats_record(w, valid && g == 0, lane, a.partials + tile * CMCD_NSTATS);
}

// ------------------------------------------------------------------------------------------
// launcher (cmcd_host.h): the instance table of cmcd_ldvi.hip's ldvi_traj_pick, the launch rule of ldvi_launch
// ------------------------------------------------------------------------------------------
typedef void (*reverse_ldvi_fn)(ReverseLdviArgs);

template <int TARGET, int D>
static reverse_ldvi_fn reverse_ldvi_pick(int T, bool net) {
  if (!net) return reverse_ldvi_kernel<TARGET, D, 1, false>;
  if constexpr (D == 2) {
    if (T == 2) return reverse_ldvi_kernel<TARGET, D, 2, true>;
    if (T == 4) return reverse_ldvi_kernel<TARGET, D, 4, true>;
  } else {
    if (T == 5) return reverse_ldvi_kernel<TARGET, D, 5, true>;
  }
  return nullptr;
}

// gmm / many_gmm (d = 2) on 2 and 4 neuron tiles, the funnel (d = 10) on 5; without a network the same three (target, dim)
static reverse_ldvi_fn reverse_ldvi_fn_of(const cmcd_desc& d, int T, bool net) {
  if (net && d.arch != CMCD_ARCH_GEFFNER) return nullptr;
  if (d.target == CMCD_TARGET_GMM && d.dim == 2) return reverse_ldvi_pick<CMCD_TARGET_GMM, 2>(T, net);
  if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) return reverse_ldvi_pick<CMCD_TARGET_MANY_GMM, 2>(T, net);
  if (d.target == CMCD_TARGET_FUNNEL && d.dim == 10) return reverse_ldvi_pick<CMCD_TARGET_FUNNEL, 10>(T, net);
  return nullptr;
}

bool reverse_ldvi_available(const cmcd_desc& d, int T, bool use_net) { return reverse_ldvi_fn_of(d, T, use_net) != nullptr; }

int reverse_ldvi_launch(const cmcd_desc& d, const cmcd_layout& lay, const WsLayout& w, bool use_net, const int32_t* seeds,
                        const float* x, int64_t n, const float* params, float* ws, float* out_w, float* out_z0, float* out_rho0,
                        hipStream_t stream) {
  const int D = d.dim, HP = w.HP;
  reverse_ldvi_fn fn = reverse_ldvi_fn_of(d, w.T, use_net);
  if (!fn) return fail(CMCD_ERR_UNSUPPORTED, "no LDVI reverse-chain kernel instance for this (target, dim, arch, width=%s%lld)", "", HP);
  const int64_t tiles = (n + 15) / 16;
  ReverseLdviArgs a{seeds, x, params, ws, reinterpret_cast<double*>(ws + w.partials), out_w, out_z0, out_rho0, lay, w, n,
                    (int32_t)d.nbridges};
  const size_t lds_bytes = size_t((use_net ? HP * HP + 3 * D * HP + HP + 16 : 0) + w.tgt_floats) * 4;
  // waves per workgroup: ldvi_launch's rule (one wave per workgroup until every SIMD has one)
  const int nw = tiles <= 1024 ? 1 : (tiles <= 8192 ? 4 : 8);
  hipLaunchKernelGGL(fn, dim3(unsigned((tiles + nw - 1) / nw)), dim3(64 * nw), lds_bytes, stream, a);
  return hipGetLastError() == hipSuccess ? CMCD_OK : fail(CMCD_ERR_HIP, "LDVI reverse-chain launch failed%s");
}

}  // namespace cmcd
