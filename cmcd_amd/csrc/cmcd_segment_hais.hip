// Resumable segments of the UHA forward chain (Hamiltonian AIS, cmcd_hais.hip) on gfx950: bridges [k0, k1) from a
// caller-supplied particle state that carries the momentum BETWEEN bridges, so that the weights can be examined (and the particles
// resampled) between bridges — cmcd_segment_uha.hip for the second of the two momentum baselines.
//
// The reference has no such call; the arithmetic is the forward call's (hais_traj_kernel, reference lines ais_utils.py:7-69,
// momdist.py:13-28), cut at a bridge, and is written out in include/cmcd_hip.h (cmcd_bound_segment_hais).  Per particle, with
// s = exp(md), L = lfsteps, gU(z, b) = -(b grad log p(z) + (1 - b) grad log q(z)) (no clip), eps and eta the scalar leaves:
//
//   k0 == 0:  key chain, z_0 and rho_prev = s normal(R) exactly as hais_traj_kernel;  wpath = -log q(z_0);  gen = gen_0
//   k0  > 0:  z, rho (= rho_prev: the momentum that left bridge k0 - 1), wpath, gen = the caller's state
//   for i = k0 .. k1-1, the forward call's bridge i:
//             rho = eta rho_prev + sqrt(1 - eta^2) s xi_i                                (xi_i: the deviate of gen_i)
//             r = rho - eps/2 gU(z, beta_i);  z += eps r / s^2;  (L - 1) times: r -= eps gU(z, beta_i);  z += eps r / s^2
//             r -= eps/2 gU(z, beta_i)
//             wpath += log N(r; 0, s) - log N(rho; 0, s) = sum_j (rho_j^2 - r_j^2) / (2 s_j^2);  rho_prev = r
//   lg = log gamma_k1(z), NO momentum term:  gamma_K = p;  0 < k < K: log gamma_k = beta_{k-1} log p + (1 - beta_{k-1}) log q
//                          (log p = -inf — the many_gmm floor — gives lg = -inf, never 0 * inf; a NaN stays a NaN)
//   out: z, rho = rho_prev, wpath, lg, key = gen_k1;  statistics over l := -(wpath + lg)
//
// Why lg has no momentum term (include/cmcd_hip.h has the derivation): the refresh is reversible with respect to N(0, s^2), so
// the backward kernel of a refresh is the refresh, the ratio of the two is N(rho_prev; 0, s) / N(rho; 0, s), and with the
// densities of the initial and the final momentum the momentum terms telescope to prod_i N(r_i) / N(rho_i): exactly what wpath
// accumulates.  exp(wpath + lg) is then a proper weight for gamma_k(z) N(rho_prev; 0, s^2) on the pair (z, rho_prev).
//
// Segments compose bit for bit by the structure of cmcd_segment_uha.hip: ONE runtime loop over the evaluations
// m = k0 L .. k1 L with a SINGLE site that evaluates (log p, grad log p, grad log q).  The evaluation that closes one bridge
// opens the next, and at m == k1 L it forms lg: (k1 - k0) L + 1 target evaluations per segment, one extra per cut.
//
// Mapping = hais_traj_kernel's: one wave per 16-particle tile, four tiles per 256-thread workgroup, lane (g, c) = particle c;
// betas formed by every workgroup in its prologue (cmcd_mom.h: mom_form_betas), no prep launch.  z, the momenta, wpath and the
// key in registers; one statistics record per tile.  Plain vector stores only.
#include "cmcd_mom.h"

namespace cmcd {

struct SegmentHaisArgs {
  const int32_t* seeds;     // read when k0 == 0
  const float* params;
  const float* tc;          // target_consts as handed to the C ABI ({scale, means} for many_gmm)
  float* z;                 // [n][D]  in (k0 > 0) and out
  float* rho;               // [n][D]  in (k0 > 0) and out: the momentum between bridges
  float* wpath;             // [n]     in (k0 > 0) and out
  uint32_t* key;            // [n][2]  in (k0 > 0) and out: gen_k0 -> gen_k1
  float* lg;                // [n]     out
  double* partials;         // [tiles][5]
  cmcd_hais_layout lay;
  int64_t n;
  int32_t K, L, n_mix, k0, k1;   // bridges [k0, k1), 0 <= k0 < k1 <= K
};

template <int TARGET, int D>
__global__ __launch_bounds__(256) void segment_hais_kernel(SegmentHaisArgs a) {
  __shared__ __attribute__((aligned(16))) float lds_tgt[4 + 2 * 64];
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];   // betas[K], gy[ngrid + 2]
  float* betas = lds_dyn;
  if (TARGET == CMCD_TARGET_MANY_GMM) tile_stage_many_gmm(a.tc, a.n_mix, lds_tgt);
  mom_form_betas(a.params, a.lay, a.K, betas, lds_dyn + a.K);
  constexpr int Hh = (D + 1) / 2;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
  const int64_t p = tile * 16 + c;
  if (tile * 16 >= a.n) return;
  const bool valid = p < a.n;
  const int64_t pl = valid ? p : a.n - 1;   // the lanes past the batch repeat its last particle and store nothing
  const int64_t pD = p * D;
  const int ks = a.k0, ke = a.k1, K = a.K, L = a.L;

  float z[D], qmean[D], qiv[D], sm[D], iv[D], r[D], rho[D];
  float nz[2 * Hh];
  uint32_t k0, k1;
  float w = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float sd = expf(a.params[a.lay.vd_logdiag + j]);
    qmean[j] = a.params[a.lay.vd_mean + j];
    qiv[j] = 1.0f / (sd * sd);
    sm[j] = expf(a.params[a.lay.md + j]);
    iv[j] = 1.0f / (sm[j] * sm[j]);
    rho[j] = 0.f;
  }
  if (ks == 0) {
    // ---- the forward call's start (boundingmachine.py:84-93, ais_utils.py:62-66): (A, B) = split(PRNGKey(seed));
    // z_0 = mean + std normal(A); C = first(split(B)); (R, G') = split(C); rho_prev = s normal(R); gen_0 = second(split(G'))
    const int gb = g & 1;
    const int32_t seed = a.seeds[pl];
    uint32_t x0, x1, a0, a1, b0, b1;
    tile_split(0u, (uint32_t)seed, gb, x0, x1);
    rows01(x0, a0, a1);
    rows01(x1, b0, b1);
    tile_normal<D>(a0, a1, g, nz);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float mean = qmean[j], sd = expf(a.params[a.lay.vd_logdiag + j]);
      z[j] = sd * nz[j] + mean;
      const float dz = z[j] - mean;
      w -= -(dz * dz) / (2.0f * sd * sd) - logf(sd) - kHalfLog2Pi;   // wpath = -log q(z_0)
    }
    tile_split(b0, b1, gb, x0, x1);
    uint32_t c0, c1;
    rows01(x0, c0, c1);
    tile_split(c0, c1, gb, x0, x1);
    uint32_t r0, r1, p0, p1;
    rows01(x0, r0, r1);
    rows01(x1, p0, p1);
    tile_normal<D>(r0, r1, g, nz);
#pragma unroll
    for (int j = 0; j < D; ++j) r[j] = sm[j] * nz[j];
    tile_split(p0, p1, gb, x0, x1);
    rows01(x1, k0, k1);
  } else {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      z[j] = a.z[pl * D + j];
      r[j] = a.rho[pl * D + j];
    }
    w = a.wpath[pl];
    k0 = a.key[pl * 2];
    k1 = a.key[pl * 2 + 1];
  }

  const float eps = a.params[a.lay.eps], eta = a.params[a.lay.eta];
  const float ce = sqrtf(1.0f - eta * eta);
  const int m0 = ks * L, M = ke * L;
  float logp = 0.f;
  int i = ks, l = 0;   // evaluation m opens step l of bridge i (l == 0 and m > m0: it also closes bridge i - 1)
  for (int m = m0;; ++m) {
    float gp[D], gq[D];
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
#pragma unroll
    for (int j = 0; j < D; ++j) gq[j] = -(z[j] - qmean[j]) * qiv[j];
    if (m > m0 && l == 0) {   // the closing half kick of bridge i - 1 and its weight
      const float bp = betas[i - 1];
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float gU = -1.0f * (bp * gp[j] + (1.0f - bp) * gq[j]);
        r[j] -= 0.5f * eps * gU;
        acc += (rho[j] - r[j]) * (rho[j] + r[j]) * iv[j];
      }
      w += 0.5f * acc;
    }
    if (m == M) break;
    const float be = betas[i];
    if (l == 0) {
      tile_chain_step<D>(k0, k1, g, nz);   // (G, H) = split(gen); xi_i = normal(G); gen = second(split(H))
#pragma unroll
      for (int j = 0; j < D; ++j) {
        rho[j] = eta * r[j] + ce * sm[j] * nz[j];
        const float gU = -1.0f * (be * gp[j] + (1.0f - be) * gq[j]);
        r[j] = rho[j] - 0.5f * eps * gU;
      }
    } else {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float gU = -1.0f * (be * gp[j] + (1.0f - be) * gq[j]);
        r[j] -= eps * gU;
      }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] += eps * r[j] * iv[j];
    if (++l == L) { l = 0; ++i; }
  }

  // lg = log gamma_k1(z_k1): log p at the end of the chain, the geometric bridge of bridge k1 - 1 before it; no momentum term
  float lg = logp;
  if (ke < K) {
    float logq = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float sd = expf(a.params[a.lay.vd_logdiag + j]);
      const float dz = z[j] - qmean[j];
      logq += -(dz * dz) / (2.0f * sd * sd) - logf(sd) - kHalfLog2Pi;
    }
    const float bl = betas[ke - 1];
    lg = (logp == -INFINITY) ? -INFINITY : bl * logp + (1.0f - bl) * logq;
  }
  const float loss = -(w + lg);

  if (valid && g == 0) {
    a.wpath[p] = w;
    a.lg[p] = lg;
    a.key[p * 2] = k0;
    a.key[p * 2 + 1] = k1;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      a.z[pD + j] = z[j];
      a.rho[pD + j] = r[j];
    }
  }
  tile_stats_record(loss, valid && g == 0, lane, a.partials + tile * CMCD_NSTATS);
}

// ------------------------------------------------------------------------------------------
// launcher (cmcd_host.h): the instances and the shape limits of cmcd_hais.hip (tile_pick_plain, hais_shape_ok)
// ------------------------------------------------------------------------------------------
struct SegmentHais {
  typedef void (*fn)(SegmentHaisArgs);
  template <int TARGET, int D> static fn get() { return segment_hais_kernel<TARGET, D>; }
};

bool segment_hais_available(int target, int dim) { return tile_pick_plain<SegmentHais>(target, dim) != nullptr; }

int segment_hais_launch(int target, int dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout& lay, int32_t k0, int32_t k1,
                        const int32_t* seeds, int64_t n, const float* params, const float* target_consts, int n_mix, float* ws,
                        float* z, float* rho, float* wpath, uint32_t* key, float* lg, hipStream_t stream) {
  SegmentHais::fn fn = tile_pick_plain<SegmentHais>(target, dim);
  if (!fn) return fail(CMCD_ERR_UNSUPPORTED, "no Hamiltonian AIS segment kernel instance for this (target, dim)%s");
  const int64_t tiles = (n + 15) / 16;
  SegmentHaisArgs a{seeds, params, target_consts, z, rho, wpath, key, lg, reinterpret_cast<double*>(ws), lay, n, nbridges,
                    lfsteps, n_mix, k0, k1};
  const size_t lds = sizeof(float) * ((size_t)nbridges + (size_t)lay.ngrid + 2);
  hipLaunchKernelGGL(fn, dim3((unsigned)((tiles + 3) / 4)), dim3(256), lds, stream, a);
  return hipGetLastError() == hipSuccess ? CMCD_OK : fail(CMCD_ERR_HIP, "Hamiltonian AIS segment launch failed%s");
}

}  // namespace cmcd
