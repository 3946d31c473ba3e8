// The reverse-time chain of UHA (Hamiltonian AIS, cmcd_hais.hip) on gfx950: target draws get a fresh momentum and are pushed
// through the forward chain's leap-frogs run backwards; the momentum refresh rho = eta rho_prev + sqrt(1 - eta^2) s xi is
// reversible with respect to N(0, s^2), so the backward kernel of a refresh is the refresh itself.
//
// The reference has no such call; what is restated here is the arithmetic of its forward chain (hais_traj_kernel, reference
// lines ais_utils.py:7-69, momdist.py:13-28), walked the other way, and is written out in include/cmcd_hip.h
// (cmcd_bound_reverse_hais).  Per particle, with s = exp(md), L = lfsteps, gU(z, b) = -(b grad log p(z) + (1 - b) grad log q(z))
// (no clip), eps the scalar leaf:
//
//   z_K = x;  r = s normal(R);  w = log p(z_K)
//   for i = K-1 .. 0:
//     w  += log N(r; 0, s)
//     rho = r + eps gU(z, beta_i) / 2                                            ais_utils.py:51-52 undone
//     (L - 1) times:  z -= eps rho / s^2;  rho += eps gU(z, beta_i)              :45-48 undone
//     z  -= eps rho / s^2;  rho += eps gU(z, beta_i) / 2                         :38-42 undone: now (z_i, rho_i)
//     w  -= log N(rho; 0, s)
//     r   = eta rho + sqrt(1 - eta^2) s xi_r,  r = K-1-i                         the refresh, reversed
//   w -= log q(z_0)
//
// The two densities of a bridge share their normalising constant, so w takes sum_j (rho_j^2 - r_j^2) / (2 s_j^2), the opening
// half at the head of the bridge and the closing half at its end.  Key chain = the 2nd-order reverse chain's: the forward
// chain's without its first draw.  The last r — the chain's initial momentum — leaves as rho0.
//
// ONE runtime loop over the evaluations m = K L .. 0 with a single evaluation site: the evaluation that ends one bridge's
// leap-frog (closing half-kick, weight, refresh) opens the next one's (opening half-kick).  K L + 1 target evaluations.
//
// Mapping = hais_traj_kernel's: one wave per 16-particle tile, four tiles per 256-thread workgroup, lane (g, c) = particle c;
// betas formed by every workgroup in its prologue (cmcd_mom.h: mom_form_betas), no prep launch.  One statistics record per tile
// over l := w.  Plain vector stores only.  A particle whose x row holds a non-finite entry, whose log p(x) is floored (many_gmm)
// or whose w comes out NaN leaves with w = +inf (weight 0).
#include "cmcd_mom.h"

namespace cmcd {

struct ReverseHaisArgs {
  const int32_t* seeds;
  const float* x;           // [n][D] target draws
  const float* params;
  const float* tc;          // target_consts as handed to the C ABI ({scale, means} for many_gmm)
  float* out_w;
  float* out_z0;
  float* out_rho0;
  double* partials;         // [tiles][5]
  cmcd_hais_layout lay;
  int64_t n;
  int32_t K, L, n_mix;
};

template <int TARGET, int D>
__global__ __launch_bounds__(256) void reverse_hais_kernel(ReverseHaisArgs a) {
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

  float z[D], qmean[D], qiv[D], sm[D], iv[D], r[D];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float mean = a.params[a.lay.vd_mean + j], sd = expf(a.params[a.lay.vd_logdiag + j]);
    qmean[j] = mean;
    qiv[j] = 1.0f / (sd * sd);
    sm[j] = expf(a.params[a.lay.md + j]);
    iv[j] = 1.0f / (sm[j] * sm[j]);
    z[j] = a.x[pl * D + j];                        // z_K = x
    bad = bad || !isfinite(z[j]);
  }

  // key chain: (_, B) = split(PRNGKey(seed)); C = first(split(B)); (R, G') = split(C); r = s normal(R); gen_0 = second(split(G'))
  const int gb = g & 1;
  uint32_t k0, k1;
  float nz[2 * Hh];
  {
    const int32_t seed = a.seeds[pl];
    uint32_t x0, x1, b0, b1, c0, c1, r0, r1, p0, p1;
    tile_split(0u, (uint32_t)seed, gb, x0, x1);    // (A, B); A (the forward call's z_0 key) is not used
    rows01(x1, b0, b1);
    tile_split(b0, b1, gb, x0, x1);
    rows01(x0, c0, c1);
    tile_split(c0, c1, gb, x0, x1);
    rows01(x0, r0, r1);
    rows01(x1, p0, p1);
    tile_normal<D>(r0, r1, g, nz);
#pragma unroll
    for (int j = 0; j < D; ++j) r[j] = sm[j] * nz[j];
    tile_split(p0, p1, gb, x0, x1);
    rows01(x1, k0, k1);
  }

  const float eps = a.params[a.lay.eps], eta = a.params[a.lay.eta];
  const float ce = sqrtf(1.0f - eta * eta);
  const int K = a.K, L = a.L;
  const int M = K * L;
  float w = 0.f;
  int i = K, l = 0;   // i: the bridge being inverted; l: kicks of it undone so far (l == 0: evaluation m ends bridge i and opens i - 1)
  for (int m = M;; --m) {
    float gp[D], gq[D], logp;
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
#pragma unroll
    for (int j = 0; j < D; ++j) gq[j] = -(z[j] - qmean[j]) * qiv[j];
    if (m == M) {
      w = logp;                                    // w = log p(z_K)
      bad = bad || logp == -INFINITY;              // many_gmm: x under the floor of log p
    } else if (l == 0) {
      // the opening half-kick of bridge i undone: (z_i, rho_i); its weight; the refresh, reversed
      const float be = betas[i];
      tile_chain_step<D>(k0, k1, g, nz);           // (G, H) = split(gen); xi_r = normal(G); gen = second(split(H))
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float gU = -1.0f * (be * gp[j] + (1.0f - be) * gq[j]);
        r[j] += 0.5f * eps * gU;                   // rho_i
        acc += r[j] * r[j] * iv[j];                // -log N(rho_i; 0, s) without its constant
        r[j] = eta * r[j] + ce * sm[j] * nz[j];
      }
      w += 0.5f * acc;
    }
    if (m == 0) break;
    if (l == 0) {
      // bridge i - 1 opened at z_i: log N(r; 0, s) without its constant (the closing density's cancels it), and the closing
      // half-kick undone
      --i;
      const float be = betas[i];
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float gU = -1.0f * (be * gp[j] + (1.0f - be) * gq[j]);
        acc += r[j] * r[j] * iv[j];
        r[j] += 0.5f * eps * gU;
      }
      w -= 0.5f * acc;
    } else {
      const float be = betas[i];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float gU = -1.0f * (be * gp[j] + (1.0f - be) * gq[j]);
        r[j] += eps * gU;
      }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] -= eps * r[j] * iv[j];
    if (++l == L) l = 0;
  }

  // w -= log q(z_0)
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float sd = expf(a.params[a.lay.vd_logdiag + j]);
    const float dz = z[j] - qmean[j];
    w -= -(dz * dz) / (2.0f * sd * sd) - logf(sd) - kHalfLog2Pi;
  }
  if (bad || w != w) w = INFINITY;   // weight exp(-w) = 0, like a diverged particle's loss of the forward call

  if (valid && g == 0) {
    a.out_w[p] = w;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      a.out_z0[pD + j] = z[j];
      a.out_rho0[pD + j] = r[j];
    }
  }
  tile_stats_record(w, valid && g == 0, lane, a.partials + tile * CMCD_NSTATS);
}

// ------------------------------------------------------------------------------------------
// launcher (cmcd_host.h): the instances and the shape limits of cmcd_hais.hip (tile_pick_plain, hais_shape_ok)
// ------------------------------------------------------------------------------------------
struct ReverseHais {
  typedef void (*fn)(ReverseHaisArgs);
  template <int TARGET, int D> static fn get() { return reverse_hais_kernel<TARGET, D>; }
};

bool reverse_hais_available(int target, int dim) { return tile_pick_plain<ReverseHais>(target, dim) != nullptr; }

bool reverse_hais_shape_ok(int32_t nbridges, int32_t lfsteps, int64_t n) {
  return nbridges >= 1 && lfsteps >= 1 && n >= 1 && n <= ((int64_t)1 << 31) && nbridges <= 4096 &&
         (int64_t)nbridges * lfsteps <= ((int64_t)1 << 24);
}

// one statistics record per 16-particle tile, nothing else
int64_t reverse_hais_floats(int64_t n) { return al4(((n + 15) / 16) * CMCD_NSTATS * 2); }

int reverse_hais_launch(int target, int dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout& lay, const int32_t* seeds,
                        const float* x, int64_t n, const float* params, const float* target_consts, int n_mix, float* ws,
                        float* out_w, float* out_z0, float* out_rho0, hipStream_t stream) {
  ReverseHais::fn fn = tile_pick_plain<ReverseHais>(target, dim);
  if (!fn) return fail(CMCD_ERR_UNSUPPORTED, "no Hamiltonian AIS reverse-chain kernel instance for this (target, dim)%s");
  const int64_t tiles = (n + 15) / 16;
  ReverseHaisArgs a{seeds, x, params, target_consts, out_w, out_z0, out_rho0, reinterpret_cast<double*>(ws), lay, n, nbridges,
                    lfsteps, n_mix};
  const size_t lds = sizeof(float) * ((size_t)nbridges + (size_t)lay.ngrid + 2);
  hipLaunchKernelGGL(fn, dim3((unsigned)((tiles + 3) / 4)), dim3(256), lds, stream, a);
  return hipGetLastError() == hipSuccess ? CMCD_OK : fail(CMCD_ERR_HIP, "Hamiltonian AIS reverse-chain launch failed%s");
}

}  // namespace cmcd
