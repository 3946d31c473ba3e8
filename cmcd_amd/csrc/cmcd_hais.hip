// UHA — Hamiltonian AIS (uncorrected Hamiltonian annealing): the reference's plain bounding machine with nbridges >= 1
// (/root/reference/src/boundingmachine.py:73-111 -> ais_utils.py:7-69 -> momdist.py:13-28), its bound and the reparameterised
// gradient of the mean bound.  No network: target gradients, Threefry and a leap-frog.  Per seed, with s = exp(md),
// L = lfsteps and gU(z, beta) = -(beta grad log p(z) + (1 - beta) grad log q(z)) (no clip in this mode):
//
//   (A, B) = split(PRNGKey(seed));  z = mean + exp(logdiag) normal(A);  w = -log q(z)            boundingmachine.py:84-88
//   C = first(split(B));  (R, G') = split(C);  rho_prev = s normal(R);  gen = second(split(G'))   :93, ais_utils.py:62-66
//   bridge i = 0 .. K-1:
//     (G, H) = split(gen);  xi = normal(G);  gen = second(split(H))                               ais_utils.py:15,21
//     rho = eta rho_prev + sqrt(1 - eta^2) s xi                                                   momdist.py:13-21
//     r = rho - eps/2 gU(z, beta_i);  z += eps r / s^2                                            ais_utils.py:38-42
//     (L - 1) times:  r -= eps gU(z, beta_i);  z += eps r / s^2                                   :30-35,45-48
//     r -= eps/2 gU(z, beta_i)                                                                    :51-52
//     w += log N(r; 0, s) - log N(rho; 0, s) = sum_j (rho_j^2 - r_j^2) / (2 s_j^2);  rho_prev = r :20
//   w += log p(z);  loss = -w                                                                     boundingmachine.py:100-103
//
// The closing half kick of bridge i and the opening one of bridge i + 1 sit at the same z: K L + 1 target evaluations per particle,
// walked by ONE runtime loop over the evaluations m = 0 .. K L with a single evaluation site (K and L are runtime values).
// beta_i = interp(target_x, gridref_x, [0, cumsum(mgridref_y) / sum]) (boundingmachine.py:79-82) is formed by every workgroup in its
// prologue into LDS, straight from params_flat: no prep launch.  delta_H (ais_utils.py:55) is dropped by compute_bound and not
// produced.
//
// Mapping (cmcd_mfvi.hip's and ula_grad_kernel's): one wave per 16-particle tile, four tiles per 256-thread workgroup, lane (g, c)
// = particle c; the four lanes of a particle share the target evaluation (Target<>::eval) and the Threefry blocks, and repeat
// the rest.  z, r, rho, w and the key stay in registers for the whole chain.  One 5-double statistics record per tile.
// The key split, the normal(key, (D,)) draw, the step of the key chain, the statistics record, many_gmm's constant staging and
// the instance table are cmcd_tile.h's, shared with grad_kernel and the reverse and segment kernels (mfvi_kernel keeps inline
// copies of its own, see the note above it); what is
// here is the chain itself, its reverse sweep, the beta table and the reduction.
//
// What a gradient call keeps (hais_traj_kernel with `keep`), all [.][n][D] float32 in the workspace:
//   pos  [K L + 1]  the position of every evaluation (pos[0] = z_0, pos[K L] = z_K)
//   rho  [K]        the refreshed momentum of every bridge
//   rend [K + 1]    rend[0] = s normal(R), rend[i + 1] = the momentum that leaves bridge i (what the next refresh starts from)
// The reverse sweep (hais_grad_kernel) walks the evaluations backwards carrying the adjoints of z and r; the momentum between two
// kicks is recovered from rend by undoing the kicks (r_before = r_after + kappa gU), the deviates from rho - eta rho_prev.  Every
// per-tile partial {d mean[D], d logdiag[D], d md[D], d eps, d eta, d beta[K]} goes to a slot of its own with plain stores;
// hais_reduce_kernel (one workgroup) sums the tiles in a fixed order and carries d beta through the interpolation and the
// normalised cumulative sum into mgridref_y.  No float atomics: repeated calls return the same bits.
//
// lgcp (d = 1600) does not fit this mapping (a particle's state in registers): cmcd_hais_lgcp.hip runs the same arithmetic as one
// launch per target evaluation, behind cmcd_hais_lgcp_bound_grad; the entry points here keep refusing it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cmcd_tile.h"

namespace cmcd {

constexpr int kHaisMaxBridges = 4096;   // 3 K floats of dynamic LDS in the reduction launch
constexpr int kHaisMaxGrid = 1024;      // ngrid: the grid nodes sit next to the betas in LDS

struct HaisArgs {
  const int32_t* seeds;
  const float* params;
  const float* tc;          // target_consts as handed to the C ABI ({scale, means} for many_gmm)
  float* out_loss;
  float* out_z;
  double* partials;         // [tiles][5]
  float* pos;               // kept trajectory (forward: written when non-null; sweep: read)
  float* rho;
  float* rend;
  float* gpart;             // [tiles][3 D + 2 + K] (sweep)
  cmcd_hais_layout lay;
  int64_t n;
  int32_t K, L, n_mix;
  float omega;
};

// cell of np.interp for abscissa x on the grid gx[0 .. G + 1]: searchsorted(gx, x, side = 'right') clipped to [1, G + 1]
__device__ __forceinline__ int hais_cell(const float* gx, int G, float x) {
  int j = 1;
  while (j < G + 1 && gx[j] <= x) ++j;
  return j;
}

// betas[K] from mgridref_y; gy[G + 2] = [0, cumsum(m) / sum(m)] is left in LDS next to them.  Ends with a barrier.
__device__ __forceinline__ void hais_form_betas(const HaisArgs& a, float* betas, float* gy) {
  const int G = (int)a.lay.ngrid;
  const float* m = a.params + a.lay.mgridref_y;
  const float* gx = a.params + a.lay.gridref_x;
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
  for (int i = threadIdx.x; i < a.K; i += blockDim.x) {
    const float x = a.params[a.lay.target_x + i];
    const int j = hais_cell(gx, G, x);
    betas[i] = gy[j - 1] + ((x - gx[j - 1]) / (gx[j] - gx[j - 1])) * (gy[j] - gy[j - 1]);
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------
// forward chain
// ------------------------------------------------------------------------------------------
template <int TARGET, int D>
__global__ __launch_bounds__(256) void hais_traj_kernel(HaisArgs a) {
  __shared__ __attribute__((aligned(16))) float lds_tgt[4 + 2 * 64];
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];   // betas[K], gy[ngrid + 2]
  float* betas = lds_dyn;
  if (TARGET == CMCD_TARGET_MANY_GMM) tile_stage_many_gmm(a.tc, a.n_mix, lds_tgt);
  hais_form_betas(a, betas, lds_dyn + a.K);
  constexpr int Hh = (D + 1) / 2;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
  const int64_t p = tile * 16 + c;
  if (tile * 16 >= a.n) return;
  const bool valid = p < a.n;
  const bool keep = a.pos != nullptr && valid && g == 0;
  const int32_t seed = a.seeds[valid ? p : a.n - 1];
  const int64_t nD = a.n * D, pD = p * D;

  // key chain up to the first bridge
  const int gb = g & 1;
  uint32_t x0, x1, a0, a1, b0, b1;
  tile_split(0u, (uint32_t)seed, gb, x0, x1);
  rows01(x0, a0, a1);
  rows01(x1, b0, b1);
  float nz[2 * Hh];
  tile_normal<D>(a0, a1, g, nz);                   // z_0 = mean + std normal(A)
  float z[D], qmean[D], qiv[D], sm[D], iv[D], r[D], rho[D];
  float w = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float mean = a.params[a.lay.vd_mean + j], ld = a.params[a.lay.vd_logdiag + j];
    const float sd = expf(ld);
    z[j] = sd * nz[j] + mean;
    const float dz = z[j] - mean;
    w -= -(dz * dz) / (2.0f * sd * sd) - logf(sd) - kHalfLog2Pi;   // w = -log q(z)
    qmean[j] = mean;
    qiv[j] = 1.0f / (sd * sd);
    sm[j] = expf(a.params[a.lay.md + j]);
    iv[j] = 1.0f / (sm[j] * sm[j]);
  }
  tile_split(b0, b1, gb, x0, x1);                  // C = first(split(B))
  uint32_t c0, c1;
  rows01(x0, c0, c1);
  tile_split(c0, c1, gb, x0, x1);                  // (R, G') = split(C)
  uint32_t r0, r1, p0, p1;
  rows01(x0, r0, r1);
  rows01(x1, p0, p1);
  tile_normal<D>(r0, r1, g, nz);                   // rho_prev = s normal(R)
#pragma unroll
  for (int j = 0; j < D; ++j) {
    r[j] = sm[j] * nz[j];
    rho[j] = r[j];
  }
  tile_split(p0, p1, gb, x0, x1);                  // gen = second(split(G'))
  uint32_t k0, k1;
  rows01(x1, k0, k1);
  if (keep) {
#pragma unroll
    for (int j = 0; j < D; ++j) a.rend[pD + j] = r[j];
  }

  const float eps = a.params[a.lay.eps], eta = a.params[a.lay.eta];
  const float ce = sqrtf(1.0f - eta * eta);
  const int K = a.K, L = a.L;
  const int M = K * L;
  float logp = 0.f;
  int i = 0, l = 0;   // evaluation m opens step l of bridge i (l == 0: it also closes bridge i - 1)
  for (int m = 0;; ++m) {
    if (keep) {
#pragma unroll
      for (int j = 0; j < D; ++j) a.pos[(int64_t)m * nD + pD + j] = z[j];
    }
    float gp[D], gq[D];
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
#pragma unroll
    for (int j = 0; j < D; ++j) gq[j] = -(z[j] - qmean[j]) * qiv[j];
    if (m > 0 && l == 0) {   // the closing half kick of bridge i - 1 and its weight
      const float bp = betas[i - 1];
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float gU = -1.0f * (bp * gp[j] + (1.0f - bp) * gq[j]);
        r[j] -= 0.5f * eps * gU;
        acc += (rho[j] - r[j]) * (rho[j] + r[j]) * iv[j];
      }
      w += 0.5f * acc;
      if (keep) {
#pragma unroll
        for (int j = 0; j < D; ++j) a.rend[(int64_t)i * nD + pD + j] = r[j];
      }
    }
    if (m == M) break;
    const float be = betas[i];
    if (l == 0) {
      tile_chain_step<D>(k0, k1, g, nz);
#pragma unroll
      for (int j = 0; j < D; ++j) {
        rho[j] = eta * r[j] + ce * sm[j] * nz[j];
        const float gU = -1.0f * (be * gp[j] + (1.0f - be) * gq[j]);
        r[j] = rho[j] - 0.5f * eps * gU;
      }
      if (keep) {
#pragma unroll
        for (int j = 0; j < D; ++j) a.rho[(int64_t)i * nD + pD + j] = rho[j];
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
  w += logp;
  const float loss = -w;
  if (valid && g == 0) {
    a.out_loss[p] = loss;
#pragma unroll
    for (int j = 0; j < D; ++j) a.out_z[pD + j] = z[j];
  }
  tile_stats_record(loss, valid && g == 0, lane, a.partials + tile * CMCD_NSTATS);
}

// ------------------------------------------------------------------------------------------
// reverse sweep over the kept evaluations.  With lb = omega (the adjoint of every loss), zb / rb the adjoints of the position
// and of the momentum that leaves evaluation m, evaluation m is undone in the order drift, opening kick (and, at the head of
// a bridge, the refresh and its weight term), closing kick of the previous bridge (and its weight term); the target Hessian
// and q's closed-form one then take the adjoints of grad log p / grad log q back to the position.
// ------------------------------------------------------------------------------------------
template <int TARGET, int D>
__global__ __launch_bounds__(256) void hais_grad_kernel(HaisArgs a) {
  __shared__ __attribute__((aligned(16))) float lds_tgt[4 + 2 * 64];
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
  float* betas = lds_dyn;
  if (TARGET == CMCD_TARGET_MANY_GMM) tile_stage_many_gmm(a.tc, a.n_mix, lds_tgt);
  hais_form_betas(a, betas, lds_dyn + a.K);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
  if (tile * 16 >= a.n) return;
  const int64_t p = tile * 16 + c;
  const bool valid = p < a.n;
  const int64_t pc = valid ? p : a.n - 1;
  const float om = valid ? a.omega : 0.f;
  const int64_t nD = a.n * D, pD = pc * D;
  const int K = a.K, L = a.L, M = K * L;
  const int64_t rowlen = 3 * D + 2 + K;
  float* out = a.gpart + tile * rowlen;
  float qmean[D], qiv[D], iv[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    qmean[j] = a.params[a.lay.vd_mean + j];
    const float sd = expf(a.params[a.lay.vd_logdiag + j]);
    qiv[j] = 1.0f / (sd * sd);
    const float s = expf(a.params[a.lay.md + j]);
    iv[j] = 1.0f / (s * s);
  }
  const float eps = a.params[a.lay.eps], eta = a.params[a.lay.eta];
  const float ic2 = 1.0f / (1.0f - eta * eta);
  constexpr int HN = Target<TARGET, D>::HN;
  float zb[D], rb[D], r[D], gmu[D], glam[D], gmd[D];
#pragma unroll
  for (int j = 0; j < D; ++j) { zb[j] = 0.f; rb[j] = 0.f; r[j] = 0.f; gmu[j] = 0.f; glam[j] = 0.f; gmd[j] = 0.f; }
  float geps = 0.f, geta = 0.f, gb_acc = 0.f;
  int i = K, l = 0;   // evaluation m = i L + l
  for (int m = M; m >= 0; --m) {
    float z[D], gp[D], gq[D], hs[HN], logp;
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = a.pos[(int64_t)m * nD + pD + j];
    Target<TARGET, D>::eval_hess(z, g, lds_tgt, logp, gp, hs);
#pragma unroll
    for (int j = 0; j < D; ++j) gq[j] = -(z[j] - qmean[j]) * qiv[j];
    float a_gp[D], a_gq[D], re[D];
#pragma unroll
    for (int j = 0; j < D; ++j) { a_gp[j] = 0.f; a_gq[j] = 0.f; re[j] = 0.f; }
    if (l == 0) {
#pragma unroll
      for (int j = 0; j < D; ++j) re[j] = a.rend[(int64_t)i * nD + pD + j];   // what enters bridge i = what left bridge i - 1
    }
    if (m < M) {
      const float be = betas[i];
      const float kap = l == 0 ? 0.5f * eps : eps, kf = l == 0 ? 0.5f : 1.0f;
      float sb = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float gU = -1.0f * (be * gp[j] + (1.0f - be) * gq[j]);
        // drift z' = z + eps r / s^2 with r = the momentum after this evaluation's kick
        const float t = zb[j] * r[j] * iv[j];
        rb[j] += eps * iv[j] * zb[j];
        geps += t;
        gmd[j] -= 2.0f * eps * t;
        // kick r = r_in - kap gU
        a_gp[j] += be * kap * rb[j];
        a_gq[j] += (1.0f - be) * kap * rb[j];
        sb += (gp[j] - gq[j]) * rb[j];
        geps -= kf * gU * rb[j];
        r[j] += kap * gU;          // the momentum before the kick (l > 0: what the previous evaluation's drift used)
      }
      gb_acc += kap * sb;
      if (l == 0) {
        // refresh rho = eta rho_prev + sqrt(1 - eta^2) s xi and the weight term -rho^2 / (2 s^2) of the loss
        const float tb = row_sum16(gb_acc);
        if (lane == 0) out[3 * D + 2 + i] = tb;
        gb_acc = 0.f;
#pragma unroll
        for (int j = 0; j < D; ++j) {
          const float rh = a.rho[(int64_t)i * nD + pD + j];
          const float rhob = rb[j] - om * rh * iv[j];
          gmd[j] += om * rh * rh * iv[j];
          const float dv = rh - eta * re[j];          // sqrt(1 - eta^2) s xi
          geta += rhob * (re[j] - eta * ic2 * dv);
          gmd[j] += rhob * dv;
          rb[j] = eta * rhob;
          if (m == 0) gmd[j] += rb[j] * re[j];        // rend[0] = s normal(R)
        }
      }
    }
    if (m > 0 && l == 0) {   // closing half kick of bridge i - 1: r_end = r - eps/2 gU, loss += r_end^2 / (2 s^2)
      const float bp = betas[i - 1];
      float sb = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float gU = -1.0f * (bp * gp[j] + (1.0f - bp) * gq[j]);
        rb[j] += om * re[j] * iv[j];
        gmd[j] -= om * re[j] * re[j] * iv[j];
        a_gp[j] += bp * 0.5f * eps * rb[j];
        a_gq[j] += (1.0f - bp) * 0.5f * eps * rb[j];
        sb += (gp[j] - gq[j]) * rb[j];
        geps -= 0.5f * gU * rb[j];
        r[j] = re[j] + 0.5f * eps * gU;
      }
      gb_acc += 0.5f * eps * sb;
    }
    float hv[D];
    Target<TARGET, D>::hvp(hs, z, a_gp, hv);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      if (m == M) zb[j] -= om * gp[j];               // loss -= log p(z_K)
      zb[j] += hv[j] - a_gq[j] * qiv[j];
      gmu[j] += a_gq[j] * qiv[j];
      glam[j] += a_gq[j] * (-2.0f * gq[j]);
      if (m == 0) {   // z_0 = mean + std e,  log q(z_0) = -|e|^2 / 2 - sum logdiag - const
        gmu[j] += zb[j];
        glam[j] += zb[j] * (z[j] - qmean[j]) - om;
      }
    }
    if (l == 0) { l = L - 1; --i; } else --l;
  }
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float tm = row_sum16(gmu[j]), tl = row_sum16(glam[j]), td = row_sum16(gmd[j]);
    if (lane == 0) {
      out[j] = tm;
      out[D + j] = tl;
      out[2 * D + j] = td;
    }
  }
  const float te = row_sum16(geps), tt = row_sum16(geta);
  if (lane == 0) {
    out[3 * D] = te;
    out[3 * D + 1] = tt;
  }
}

// ------------------------------------------------------------------------------------------
// one workgroup: zero grad, fixed-order sums of the per-tile rows, d beta -> d mgridref_y
// ------------------------------------------------------------------------------------------
struct HaisReduceArgs {
  const float* params;
  const float* rows;      // [tiles][3 D + 2 + K]
  float* grad;            // [n_params]
  cmcd_hais_layout lay;
  int64_t tiles, n_params;
  int32_t K, D;
};

__global__ __launch_bounds__(256) void hais_reduce_kernel(HaisReduceArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];   // gbeta[K], frac[K], cell[K], ggy[G + 2], gy[G + 2]
  const int K = a.K, D = a.D, G = (int)a.lay.ngrid;
  float* gbeta = lds_dyn;
  float* frac = lds_dyn + K;
  int* cell = reinterpret_cast<int*>(lds_dyn + 2 * K);
  float* ggy = lds_dyn + 3 * K;
  float* gy = ggy + (G + 2);
  for (int64_t o = threadIdx.x; o < a.n_params; o += blockDim.x) a.grad[o] = 0.f;
  __syncthreads();
  const int64_t rowlen = 3 * D + 2 + K;
  for (int64_t o = threadIdx.x; o < rowlen; o += blockDim.x) {
    float acc[8];   // eight loads in flight; tile t goes to chain t % 8, the chains are added in a fixed tree
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.f;
    int64_t t = 0;
    for (; t + 8 <= a.tiles; t += 8) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = a.rows[(t + u) * rowlen + o];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += x[u];
    }
    for (; t < a.tiles; ++t) acc[0] += a.rows[t * rowlen + o];
    const float v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    if (o < D) a.grad[a.lay.vd_mean + o] = v;
    else if (o < 2 * D) a.grad[a.lay.vd_logdiag + (o - D)] = v;
    else if (o < 3 * D) a.grad[a.lay.md + (o - 2 * D)] = v;
    else if (o == 3 * D) a.grad[a.lay.eps] = v;
    else if (o == 3 * D + 1) a.grad[a.lay.eta] = v;
    else gbeta[o - (3 * D + 2)] = v;
  }
  // beta_i = gy[j - 1] + frac_i (gy[j] - gy[j - 1]),  gy = [0, cumsum(m) / sum(m)]
  const float* gx = a.params + a.lay.gridref_x;
  const float* ms = a.params + a.lay.mgridref_y;
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    const float x = a.params[a.lay.target_x + i];
    const int j = hais_cell(gx, G, x);
    cell[i] = j;
    frac[i] = (x - gx[j - 1]) / (gx[j] - gx[j - 1]);
  }
  __syncthreads();
  for (int q = threadIdx.x; q <= G + 1; q += blockDim.x) {   // node q gathers its bridges in bridge order
    float v = 0.f;
    for (int i = 0; i < K; ++i) {
      const int j = cell[i];
      if (j == q) v += frac[i] * gbeta[i];
      else if (j - 1 == q) v += (1.0f - frac[i]) * gbeta[i];
    }
    ggy[q] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float run = 0.f;
    gy[0] = 0.f;
    for (int q = 0; q <= G; ++q) {
      run += ms[q];
      gy[q + 1] = run;
    }
    const float S = run;
    float dot = 0.f;
    for (int q = 1; q <= G + 1; ++q) dot += ggy[q] * (gy[q] / S);
    // gy[q] = C_q / S with C_q = m_0 + .. + m_{q-1}:  d / d m_r = (sum_{q > r} ggy[q] - sum_q ggy[q] gy[q]) / S
    float suffix = 0.f;
    for (int rr = G; rr >= 0; --rr) {
      suffix += ggy[rr + 1];
      a.grad[a.lay.mgridref_y + rr] = (suffix - dot) / S;
    }
  }
}

struct HaisTraj {
  typedef void (*fn)(HaisArgs);
  template <int TARGET, int D> static fn get() { return hais_traj_kernel<TARGET, D>; }
};
struct HaisSweep {
  typedef void (*fn)(HaisArgs);
  template <int TARGET, int D> static fn get() { return hais_grad_kernel<TARGET, D>; }
};

struct HaisWs {
  int64_t partials, pos, rho, rend, gpart, total;   // offsets in floats
};
static HaisWs hais_ws(int dim, int K, int L, int64_t n, bool with_grad) {
  const int64_t tiles = (n + 15) / 16;
  HaisWs w{};
  w.partials = 0;
  w.pos = al4(tiles * CMCD_NSTATS * 2);
  w.total = w.pos;
  if (with_grad) {
    w.rho = w.pos + al4(((int64_t)K * L + 1) * n * dim);
    w.rend = w.rho + al4((int64_t)K * n * dim);
    w.gpart = w.rend + al4((int64_t)(K + 1) * n * dim);
    w.total = w.gpart + al4(tiles * (3 * (int64_t)dim + 2 + K));
  }
  return w;
}

static bool hais_shape_ok(int32_t nbridges, int32_t lfsteps, int64_t n) {
  return nbridges >= 1 && lfsteps >= 1 && n >= 1 && n <= ((int64_t)1 << 31) && nbridges <= kHaisMaxBridges &&
         (int64_t)nbridges * lfsteps <= ((int64_t)1 << 24);
}

}  // namespace cmcd

using namespace cmcd;

extern "C" {

int64_t cmcd_hais_workspace_bytes(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, int64_t n, int32_t with_grad) {
  if (!hais_shape_ok(nbridges, lfsteps, n) || dim < 1) return 0;
  if (target == CMCD_TARGET_LGCP) {
    fail_msg(CMCD_ERR_UNSUPPORTED, "UHA on lgcp is not served by this entry point: use cmcd_hais_lgcp_bound_grad (cmcd_hais_lgcp.hip)");
    return 0;
  }
  if (!tile_pick_plain<HaisTraj>(target, dim)) {
    fail_msg(CMCD_ERR_UNSUPPORTED, "no Hamiltonian AIS kernel instance for this (target, dim)");
    return 0;
  }
  return hais_ws(dim, nbridges, lfsteps, n, with_grad != 0).total * 4;
}

int cmcd_hais_bound_grad(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout* lay,
                         const int32_t* seeds, int64_t n, const float* params, int64_t n_params, const float* target_consts,
                         int64_t n_target, float omega, void* workspace, int64_t workspace_bytes, float* out_loss, float* out_z,
                         double* out_stats, float* grad, void* stream_) {
  if (!lay || !seeds || !params || !workspace || !out_loss || !out_z || !out_stats)
    return fail_msg(CMCD_ERR_BAD_ARG, "null pointer argument");
  if (nbridges < 1 || lfsteps < 1) return fail_msg(CMCD_ERR_BAD_ARG, "nbridges and lfsteps must be >= 1");
  if (n < 1 || n > (int64_t)1 << 31 || dim < 1) return fail_msg(CMCD_ERR_BAD_ARG, "n or dim out of range");
  if (target == CMCD_TARGET_LGCP)
    return fail_msg(CMCD_ERR_UNSUPPORTED, "UHA on lgcp is not served by this entry point: use cmcd_hais_lgcp_bound_grad (cmcd_hais_lgcp.hip)");
  if (!tile_pick_plain<HaisTraj>(target, dim))
    return fail_msg(CMCD_ERR_UNSUPPORTED, "no Hamiltonian AIS kernel instance for this (target, dim)");
  if (!hais_shape_ok(nbridges, lfsteps, n))
    return fail_msg(CMCD_ERR_UNSUPPORTED, "nbridges above 4096 or nbridges * lfsteps above 2^24");
  if (lay->ngrid < 0 || lay->ngrid > kHaisMaxGrid) return fail_msg(CMCD_ERR_BAD_ARG, "ngrid out of range (0 .. 1024)");
  auto inside = [&](int64_t off, int64_t len) { return off >= 0 && off + len <= n_params; };
  if (!(inside(lay->vd_mean, dim) && inside(lay->vd_logdiag, dim) && inside(lay->eps, 1) && inside(lay->eta, 1) &&
        inside(lay->md, dim) && inside(lay->mgridref_y, lay->ngrid + 1) && inside(lay->gridref_x, lay->ngrid + 2) &&
        inside(lay->target_x, nbridges)))
    return fail_msg(CMCD_ERR_BAD_ARG, "layout offset missing or outside params_flat");
  int n_mix = 0;
  if (int rc = check_many_gmm(target, target_consts, n_target, &n_mix)) return rc;
  const HaisWs w = hais_ws(dim, nbridges, lfsteps, n, grad != nullptr);
  if (workspace_bytes < w.total * 4 || (reinterpret_cast<uintptr_t>(workspace) & 15))
    return fail_msg(CMCD_ERR_WORKSPACE, "workspace too small or not 16-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* ws = static_cast<float*>(workspace);
  const int64_t tiles = (n + 15) / 16;
  double* partials = reinterpret_cast<double*>(ws + w.partials);
  HaisArgs ha{};
  ha.seeds = seeds; ha.params = params; ha.tc = target_consts; ha.out_loss = out_loss; ha.out_z = out_z;
  ha.partials = partials;
  if (grad) { ha.pos = ws + w.pos; ha.rho = ws + w.rho; ha.rend = ws + w.rend; ha.gpart = ws + w.gpart; }
  ha.lay = *lay; ha.n = n; ha.K = nbridges; ha.L = lfsteps; ha.n_mix = n_mix; ha.omega = omega;
  const unsigned blocks = (unsigned)((tiles + 3) / 4);
  const size_t lds = sizeof(float) * ((size_t)nbridges + (size_t)lay->ngrid + 2);
  hipLaunchKernelGGL(tile_pick_plain<HaisTraj>(target, dim), dim3(blocks), dim3(256), lds, stream, ha);
  int rc = launch_finalize(partials, (int32_t)tiles, out_stats, stream_);
  if (rc != CMCD_OK) return rc;
  if (grad) {
    hipLaunchKernelGGL(tile_pick_plain<HaisSweep>(target, dim), dim3(blocks), dim3(256), lds, stream, ha);
    HaisReduceArgs ra{params, ha.gpart, grad, *lay, tiles, n_params, nbridges, dim};
    const size_t rlds = sizeof(float) * (3 * (size_t)nbridges + 2 * ((size_t)lay->ngrid + 2));
    hipLaunchKernelGGL(hais_reduce_kernel, dim3(1), dim3(256), rlds, stream, ra);
  }
  return hipGetLastError() == hipSuccess ? CMCD_OK : fail_msg(CMCD_ERR_HIP, "launch failed");
}

}  // extern "C"
