// LDVI — `MCD_U_a-lp-sn` and its network-free sibling `MCD_U_a-lp`: underdamped Langevin with an approximate momentum refresh
// (/root/reference/src/mcd_under_lp_a.py:6-87 via mcd_utils.py:83-120 from mcdboundingmachine.py:126-179), its bound and the
// reparameterised gradient of the mean bound.  The arithmetic is written out in include/cmcd_hip.h (cmcd_ldvi_bound_grad).  Per
// seed, with eta = gamma eps, sigma = sqrt(2 eta), gU(z, b) = -(b grad log p(z) + (1 - b) grad log q(z)) (no clip), eps constant:
//
//   z_0 = mean + exp(logdiag) normal(A);  w = -log q(z_0);  rho_0 = normal(R);  w -= log N(rho_0; 0, 1)
//   bridge i:  rho' = rho (1 - eta) + sigma n_i;  rho'' = rho' - eps/2 gU(z, beta_i);  z' = z + eps rho''
//              rho_new = rho'' - eps/2 gU(z', beta_i);  m_b = rho' (1 - eta) + 2 eta s([z; rho'], i)
//              w += log N(rho; m_b, sigma) - log N(rho'; m_f, sigma) = -|rho - m_b|^2 / (4 eta) + |n_i|^2 / 2
//   w += log N(rho_K; 0, 1) + log p(z_K);  loss = -w
//
// What differs from 2nd-order CMCD (cmcd_uha.hip): no network in the forward kernel, ONE evaluation per bridge, no clip, no
// schedule.  The positions and momenta never depend on the network, so
//   * d / d sn is local per (particle, bridge): s is re-evaluated at the kept (z_i, rho'_i) and back-propagated with the
//     cotangent c_i = -omega (rho_i - m_b,i) (the 2 eta of m_b and the 1 / sigma^2 of the density cancel) — independent work
//     items, ldvi_net_grad_kernel;
//   * only vd, eps, gamma and the betas take a reverse sweep, and it is network-free (ldvi_sweep_kernel, laid out like
//     hais_grad_kernel): the network enters it through v_i = J_s([z_i; rho'_i])^T c_i alone, which the item kernel leaves.
//
// Mapping (cmcd_tile.h): one wave per 16-particle tile, lane (g, c) = particle c; the network as net_pre_z / net_eval_rho of
// cmcd_uha.hip (copied here: that file is hashed for the stored counter figures), layer 2 on v_mfma_f32_16x16x4_f32 from the
// packed W2 fragments.  The per-bridge bias and residual rows, W1z, W3t, packed W2 / W2^T, the betas and many_gmm's staged
// constants come from the existing prep launch (a cmcd_desc with mode CMCD_MODE_CAIS_UHA_SN, arch geffner describes exactly this
// network; without a network: CMCD_MODE_ULA, schedule tables and target constants only).
//
// What a gradient call keeps, all [.][n][D] float32: z_0..z_K | rho_0..rho_K | rho'_0..rho'_{K-1} | (rho_i - m_b,i)_{i<K}.
// Launches of a gradient call: prep, ldvi_traj_kernel, ldvi_zero_kernel, [ldvi_net_grad_kernel], ldvi_sweep_kernel,
// ldvi_reduce_kernel, then cmcd_grad.hip's particle-independent tails (d eps and d mgridref_y from the per-bridge tables; the
// embedding table, b1 and W1[2 d:] from the per-bridge sums S / S2), finalize.  Every partial goes to a slot of its own with plain stores and is summed in a fixed
// order: no float atomics, repeated calls return the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cmcd_tile.h"

namespace cmcd {

constexpr int kLdviMaxSlabs = 512;   // workgroups (one wave each) of the item kernel = slabs of parameter-gradient partials
constexpr int kLdviPad = 17;         // row length of the [feature][particle] LDS images (16 particles + 1: conflict-free columns)

struct LdviArgs {
  const int32_t* seeds;
  const float* params;
  const float* ws;          // the prep launch's tables
  double* partials;         // [tiles][5]
  float* out_loss;
  float* out_z;
  float* keep;              // [4 K + 2][n][D] (forward: written when non-null; gradient kernels: read)
  float* vin;               // [K][n][2 D]  v_i = J_s^T c_i (item kernel writes, sweep reads); null without a network
  float* rows;              // [K][tiles][2 HP]  per item: sum_p d pre1 | sum_p d h1
  float* slabs;             // [nslabs][slab floats]
  float* gpart;             // [tiles][2 D + 2 + K]  (sweep)
  cmcd_layout lay;
  WsLayout w;
  int64_t n;
  int32_t K, nslabs;
  float omega;
};

__host__ __device__ constexpr int ldvi_tj(int D) { return (2 * D + 15) / 16; }   // 16-row tiles of the state input [z; rho']
__host__ __device__ constexpr int ldvi_slab_floats(int D, int HP) { return HP * HP + 16 * ldvi_tj(D) * HP + HP * 16 + HP + 16; }

// first-layer pre-activation of the z part: bias row (embedding folded by the prep launch) + z W1[:d]   (cmcd_uha.hip)
template <int D, int T>
__device__ __forceinline__ void ldvi_pre_z(const float (&z)[D], const float* __restrict__ brow, const float* lds_w1z, int g,
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

// s([z; rho], i) of the geffner net for the 16 particles of this wave (cmcd_uha.hip: net_eval_rho)
//   u = [z; rho; emb]; u += softplus(u W1 + b1); u += softplus(u W2 + b2); factor (u W3 + b3)      nn.py:45-52,66-70
template <int D, int T>
__device__ __forceinline__ void ldvi_eval_rho(const f32x4 (&prez)[T], const float (&z)[D], const float (&rho)[D],
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

// ------------------------------------------------------------------------------------------
// forward chain.  Dynamic LDS (no static block in front of it): NET: w2 | w1z[2 D] | w3t | b2 | b3[16] | target constants;
// without a network the target constants alone.
// ------------------------------------------------------------------------------------------
template <int TARGET, int D, int T, bool NET>
__global__ __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4) void ldvi_traj_kernel(LdviArgs a) {
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
  const int32_t seed = a.seeds[valid ? p : a.n - 1];
  const int K = a.K;
  const int64_t nD = a.n * D, pD = p * D;
  const bool keep = a.keep && valid && g == 0;
  float* tz = a.keep;
  float* trho = a.keep ? a.keep + (int64_t)(K + 1) * nD : nullptr;
  float* trhop = a.keep ? a.keep + (int64_t)(2 * K + 2) * nD : nullptr;
  float* tres = a.keep ? a.keep + (int64_t)(3 * K + 2) * nD : nullptr;

  float qmean[D], qstd[D], qiv[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    qmean[j] = a.params[a.lay.vd_mean + j];
    qstd[j] = expf(a.params[a.lay.vd_logdiag + j]);
    qiv[j] = 1.0f / (qstd[j] * qstd[j]);
  }

  // key chain up to the first bridge (mcdboundingmachine.py:151-162; mcd_under_lp_a.py:66-67,74)
  const int gb = g & 1;
  uint32_t x0, x1, a0, a1, b0, b1;
  tile_split(0u, (uint32_t)seed, gb, x0, x1);          // (A, B) = split(PRNGKey(seed))
  rows01(x0, a0, a1);
  rows01(x1, b0, b1);
  float nz[2 * Hh], z[D], rho[D];
  tile_normal<D>(a0, a1, g, nz);                       // z_0 = mean + std normal(A)
#pragma unroll
  for (int j = 0; j < D; ++j) z[j] = qstd[j] * nz[j] + qmean[j];
  tile_split(b0, b1, gb, x0, x1);                      // C = first(split(B))
  uint32_t c0, c1;
  rows01(x0, c0, c1);
  tile_split(c0, c1, gb, x0, x1);                      // (R, G') = split(C)
  uint32_t r0, r1, p0, p1;
  rows01(x0, r0, r1);
  rows01(x1, p0, p1);
  tile_normal<D>(r0, r1, g, nz);                       // rho_0 = normal(R)
#pragma unroll
  for (int j = 0; j < D; ++j) rho[j] = nz[j];
  tile_split(p0, p1, gb, x0, x1);                      // gen = second(split(G'))
  uint32_t k0, k1;
  rows01(x1, k0, k1);
  if (keep) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      tz[pD + j] = z[j];
      trho[pD + j] = rho[j];
    }
  }

  // w = -log q(z_0) - log N(rho_0; 0, 1)
  float w = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float dz = z[j] - qmean[j];
    w -= -(dz * dz) / (2.0f * qstd[j] * qstd[j]) - logf(qstd[j]) - kHalfLog2Pi;
  }
  {
    float l0 = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) l0 += -(rho[j] * rho[j]) * 0.5f - kHalfLog2Pi;
    w -= l0;
  }

  const float eps = a.params[a.lay.eps], gamma = a.params[a.lay.gamma];
  const float eta = gamma * eps;                       // :28
  const float sig = sqrtf(2.0f * eta);                 // :30
  const float inv2s2 = 1.0f / (2.0f * sig * sig), cst = logf(sig) + kHalfLog2Pi;
  const float ome = 1.0f - eta;
  const float* bias1 = a.ws + a.w.bias1;
  const float* utab = a.ws + a.w.utab;

  float gp[D], gq[D], logp;
  Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
#pragma unroll
  for (int j = 0; j < D; ++j) gq[j] = -(z[j] - qmean[j]) * qiv[j];

  for (int i = 0; i < K; ++i) {
    const float beta = a.ws[a.w.beta + i];
    tile_chain_step<D>(k0, k1, g, nz);                 // (G, H) = split(gen); n_i = normal(G); gen = second(split(H))
    float rhop[D], s[D];
    float fk_lp = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float mf = rho[j] * ome;                   // :29
      rhop[j] = mf + sig * nz[j];                      // :33
      const float df = rhop[j] - mf;
      fk_lp += -(df * df) * inv2s2 - cst;              // :54
      s[j] = 0.f;
    }
    if (NET) {
      f32x4 prez[T];
      ldvi_pre_z<D, T>(z, bias1 + (int64_t)i * HP, lds_w1z, g, prez);
      ldvi_eval_rho<D, T>(prez, z, rhop, utab + (int64_t)i * HP, lds_w2, lds_w1z, lds_b2, lds_w3t, lds_b3, lane, s);
    }
    float bk_lp = 0.f, rpp[D], res[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float mb = NET ? rhop[j] * ome + 2.0f * eta * s[j] : rhop[j] * ome;   // :41-51
      res[j] = rho[j] - mb;
      bk_lp += -(res[j] * res[j]) * inv2s2 - cst;      // :55
      const float uf = -1.0f * (beta * gp[j] + (1.0f - beta) * gq[j]);
      rpp[j] = rhop[j] - eps * uf / 2.0f;              // :35
      z[j] = z[j] + eps * rpp[j];                      // :36
    }
    w += bk_lp - fk_lp;                                // :58
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      gq[j] = -(z[j] - qmean[j]) * qiv[j];
      const float ub = -1.0f * (beta * gp[j] + (1.0f - beta) * gq[j]);
      rho[j] = rpp[j] - eps * ub / 2.0f;               // :37
    }
    if (keep) {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        tz[(int64_t)(i + 1) * nD + pD + j] = z[j];
        trho[(int64_t)(i + 1) * nD + pD + j] = rho[j];
        trhop[(int64_t)i * nD + pD + j] = rhop[j];
        tres[(int64_t)i * nD + pD + j] = res[j];
      }
    }
  }
  {
    float lK = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) lK += -(rho[j] * rho[j]) * 0.5f - kHalfLog2Pi;
    w += lK;     // + log N(rho_K; 0, 1)   :85
  }
  w += logp;     // + log p(z_K)           mcdboundingmachine.py:178
  const float loss = -w;
  if (valid && g == 0) {
    a.out_loss[p] = loss;
#pragma unroll
    for (int j = 0; j < D; ++j) a.out_z[pD + j] = z[j];
  }
  tile_stats_record(loss, valid && g == 0, lane, a.partials + tile * CMCD_NSTATS);
}

// ------------------------------------------------------------------------------------------
// network gradient: one (tile, bridge) work item per wave at a time, one wave per workgroup; workgroup b walks the items
// b, b + nslabs, ... (item = bridge * tiles + tile) and leaves ONE slab of parameter-gradient partials.
//   forward   x = [z_i; rho'_i];  pre1 = brow_i + x W1[:2d];  h1 = u0 + softplus(pre1)  (u0 = urow_i with x in front)
//             pre2 = h1 W2 + b2;  h2 = h1 + softplus(pre2);  o = h2 W3 + b3;  s = factor o
//   backward  c = -omega (rho_i - m_b,i);  d factor += c.o;  do = factor c;  dh2 = W3 do;  dp2 = dh2 sigmoid(pre2)
//             dh1 = dh2 + W2 dp2 (matrix instructions on the packed W2^T fragments);  dp1 = dh1 sigmoid(pre1)
//             v = (dh1 + W1 dp1)[:2d]   -> vin (the sweep's input cotangent at (z_i, rho'_i))
//             per item: sum_p dp1 (the bias row's gradient), sum_p dh1 (the residual row's)   -> rows
//             dW1[:2d] += x^T dp1,  dW2 += h1^T dp2,  dW3 += h2^T do: contractions over the 16 particles as fp32 matrix
//             instructions on [feature][particle] images staged in LDS;  db2 += sum_p dp2,  db3 += sum_p do
// Slab: dW2[HP][HP] | dW1[16 TJ][HP] | dW3[HP][16] | db2[HP] | {db3[D], .., d factor at 15}.
// ------------------------------------------------------------------------------------------
template <int D, int T>
__global__ __launch_bounds__(64) void ldvi_net_grad_kernel(LdviArgs a) {
  constexpr int HP = 16 * T, TJ = ldvi_tj(D), P = kLdviPad;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* XT = lds;                    // [16 TJ][P]
  float* H1T = XT + 16 * TJ * P;      // [HP][P]
  float* H2T = H1T + HP * P;
  float* P1T = H2T + HP * P;
  float* P2T = P1T + HP * P;
  float* DOT = P2T + HP * P;          // [16][P]
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  for (int i = lane; i < (16 * TJ + 4 * HP + 16) * P; i += 64) lds[i] = 0.f;   // the rows nobody writes stay zero
  __syncthreads();

  const int K = a.K;
  const int64_t tiles = (a.n + 15) / 16, items = tiles * K;
  const int64_t nD = a.n * D;
  const float* tz = a.keep;
  const float* trhop = a.keep + (int64_t)(2 * K + 2) * nD;
  const float* tres = a.keep + (int64_t)(3 * K + 2) * nD;
  const float* w1z = a.ws + a.w.w1z;
  const float* w3t = a.ws + a.w.w3t;
  const float* w2p = a.ws + a.w.w2;
  const float* w2tp = a.ws + a.w.w2t;
  const float factor = a.ws[a.w.b3 + 15];

  f32x4 gW2[T][T], gW1[TJ][T], gW3[T], gb2[T];
  float gb3[D], gfac = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    gW3[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    gb2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < T; ++u) gW2[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < TJ; ++u) gW1[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int j = 0; j < D; ++j) gb3[j] = 0.f;

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int i = (int)(item / tiles);
    const int64_t tile = item - (int64_t)i * tiles;
    const int64_t p = tile * 16 + c;
    const bool valid = p < a.n;
    const int64_t pc = valid ? p : a.n - 1;
    const float om = valid ? a.omega : 0.f;
    float x[2 * D], cv[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      x[j] = tz[(int64_t)i * nD + pc * D + j];
      x[D + j] = trhop[(int64_t)i * nD + pc * D + j];
      cv[j] = -om * tres[(int64_t)i * nD + pc * D + j];
    }
    const float* brow = a.ws + a.w.bias1 + (int64_t)i * HP;
    const float* urow = a.ws + a.w.utab + (int64_t)i * HP;
    // ---- forward, keeping what the way back needs
    f32x4 h1[T], sg1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      f32x4 pre = *reinterpret_cast<const f32x4*>(brow + 16 * t + 4 * g);
#pragma unroll
      for (int j = 0; j < 2 * D; ++j) pre += x[j] * *reinterpret_cast<const f32x4*>(w1z + j * HP + 16 * t + 4 * g);
      f32x4 u = *reinterpret_cast<const f32x4*>(urow + 16 * t + 4 * g);
      if (16 * t < 2 * D) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int nidx = 16 * t + 4 * g + r;
#pragma unroll
          for (int j = 0; j < 2 * D; ++j)
            if (j >= 16 * t && j < 16 * t + 16) u[r] = (nidx == j) ? x[j] : u[r];
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float ds;
        h1[t][r] = u[r] + softplus_both(pre[r], ds);
        sg1[t][r] = ds;
      }
    }
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = *reinterpret_cast<const f32x4*>(a.ws + a.w.b2 + 16 * t + 4 * g);
#pragma unroll
    for (int ti = 0; ti < T; ++ti) {
#pragma unroll
      for (int to = 0; to < T; ++to) {
        const f32x4 af = *reinterpret_cast<const f32x4*>(w2p + ((ti * T + to) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[r], h1[ti][r], acc[to], 0, 0, 0);
      }
    }
    f32x4 h2[T], sg2[T];
    float part[D];
#pragma unroll
    for (int j = 0; j < D; ++j) part[j] = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float ds;
        h2[t][r] = h1[t][r] + softplus_both(acc[t][r], ds);
        sg2[t][r] = ds;
      }
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w3t + j * HP + 16 * t + 4 * g);
        part[j] += h2[t][0] * wv[0] + h2[t][1] * wv[1] + h2[t][2] * wv[2] + h2[t][3] * wv[3];
      }
    }
    float dout[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float o = group_sum(part[j]) + a.ws[a.w.b3 + j];
      if (g == 0) {
        gfac += cv[j] * o;
        gb3[j] += factor * cv[j];
      }
      dout[j] = factor * cv[j];
    }
    // ---- backward
    f32x4 dp2[T], dh1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      f32x4 dh2 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < D; ++j) dh2 += dout[j] * *reinterpret_cast<const f32x4*>(w3t + j * HP + 16 * t + 4 * g);
      dh1[t] = dh2;
      dp2[t] = dh2 * sg2[t];
      gb2[t] += dp2[t];
    }
    // dh1[k] += sum_n W2[k][n] dp2[n]: w2t[(to T + ti) 64 + lane][r] = W2[16 to + c][16 ti + 4 g + r]
#pragma unroll
    for (int ti = 0; ti < T; ++ti) {
#pragma unroll
      for (int to = 0; to < T; ++to) {
        const f32x4 af = *reinterpret_cast<const f32x4*>(w2tp + ((to * T + ti) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) dh1[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[r], dp2[ti][r], dh1[to], 0, 0, 0);
      }
    }
    f32x4 dp1[T];
    float vp[2 * D];
#pragma unroll
    for (int j = 0; j < 2 * D; ++j) vp[j] = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      dp1[t] = dh1[t] * sg1[t];
#pragma unroll
      for (int j = 0; j < 2 * D; ++j) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w1z + j * HP + 16 * t + 4 * g);
        vp[j] += dp1[t][0] * wv[0] + dp1[t][1] * wv[1] + dp1[t][2] * wv[2] + dp1[t][3] * wv[3];
        if (j >= 16 * t && j < 16 * t + 16) {   // the residual path: the lane that owns neuron j adds d h1[j]
#pragma unroll
          for (int r = 0; r < 4; ++r) vp[j] += (16 * t + 4 * g + r == j) ? dh1[t][r] : 0.f;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 2 * D; ++j) {
      const float v = group_sum(vp[j]);
      if (valid && g == 0) a.vin[((int64_t)i * a.n + p) * (2 * D) + j] = v;
    }
    float* row = a.rows + item * (2 * HP);
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s1 = row_sum16(dp1[t][r]), s2 = row_sum16(dh1[t][r]);
        if (c == 0) {
          row[16 * t + 4 * g + r] = s1;
          row[HP + 16 * t + 4 * g + r] = s2;
        }
      }
    }
    // ---- the contractions over the particles
    __syncthreads();   // the previous item's reads of the images are done
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < 2 * D; ++j) XT[j * P + c] = x[j];
#pragma unroll
      for (int j = 0; j < D; ++j) DOT[j * P + c] = dout[j];
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = (16 * t + 4 * g + r) * P + c;
        H1T[o] = h1[t][r];
        H2T[o] = h2[t][r];
        P1T[o] = dp1[t][r];
        P2T[o] = dp2[t][r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pq = 4 * q + g;   // this lane's particle of k-step q: A[i = c][k = g], B[k = g][j = c]
      float aX[TJ], aH1[T], aH2[T], bP1[T], bP2[T];
#pragma unroll
      for (int u = 0; u < TJ; ++u) aX[u] = XT[(16 * u + c) * P + pq];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        aH1[t] = H1T[(16 * t + c) * P + pq];
        aH2[t] = H2T[(16 * t + c) * P + pq];
        bP1[t] = P1T[(16 * t + c) * P + pq];
        bP2[t] = P2T[(16 * t + c) * P + pq];
      }
      const float bO = DOT[c * P + pq];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        gW3[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aH2[t], bO, gW3[t], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < TJ; ++u) gW1[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aX[u], bP1[t], gW1[u][t], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < T; ++u) gW2[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aH1[u], bP2[t], gW2[u][t], 0, 0, 0);
      }
    }
  }

  // ---- this workgroup's slab: result element [r] of lane (g, c) is row 4 g + r, column c of its 16 x 16 tile
  float* slab = a.slabs + (int64_t)blockIdx.x * ldvi_slab_floats(D, HP);
  float* sW1 = slab + HP * HP;
  float* sW3 = sW1 + 16 * TJ * HP;
  float* sb2 = sW3 + HP * 16;
  float* sb3 = sb2 + HP;
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int u = 0; u < T; ++u) slab[(16 * u + 4 * g + r) * HP + 16 * t + c] = gW2[u][t][r];
#pragma unroll
      for (int u = 0; u < TJ; ++u) sW1[(16 * u + 4 * g + r) * HP + 16 * t + c] = gW1[u][t][r];
      sW3[(16 * t + 4 * g + r) * 16 + c] = gW3[t][r];
      const float s = row_sum16(gb2[t][r]);
      if (c == 0) sb2[16 * t + 4 * g + r] = s;
    }
  }
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float s = row_sum16(gb3[j]);
    if (lane == 0) sb3[j] = s;
  }
  const float sf = row_sum16(gfac);
  if (lane == 0) sb3[15] = sf;
  if (lane >= D && lane < 15) sb3[lane] = 0.f;   // the slots between db3 and d factor_sn: nobody reads them
}

// ------------------------------------------------------------------------------------------
// reverse sweep over the kept states (network-free; hais_grad_kernel's layout).  With om the adjoint of every loss, zb / rb
// the adjoints of z_{m+1} / rho''_m on entry of position m:
//   bridge m (m < K), at z_m:  drift z_{m+1} = z_m + eps rho'';  opening kick rho'' = rho' - eps/2 gU(z_m, beta_m);
//     weight |r|^2 / (4 eta), r = rho_m - m_b, m_b = (1 - eta) rho' + 2 eta s:  g_b = -om r / (2 eta), rho' += (1 - eta) g_b + v_rho,
//     z_m += v_z (v = J_s^T (2 eta g_b), from the item kernel), rho_m += -g_b;  refresh rho' = (1 - eta) rho_m + sigma n
//   bridge m - 1 (m > 0), at z_m:  closing kick rho_m = rho'' - eps/2 gU(z_m, beta_{m-1})
//   then the target Hessian and q's closed-form one take the adjoints of grad log p / grad log q back to z_m.
// d eta collects per bridge and leaves as d gamma = eps d eta, d eps += gamma d eta.
// ------------------------------------------------------------------------------------------
template <int TARGET, int D, bool NET>
__global__ __launch_bounds__(256) void ldvi_sweep_kernel(LdviArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_tgt[];
  for (int i = threadIdx.x; i < a.w.tgt_floats; i += blockDim.x) lds_tgt[i] = a.ws[a.w.tgt + i];
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
  if (tile * 16 >= a.n) return;
  const int64_t p = tile * 16 + c;
  const bool valid = p < a.n;
  const int64_t pc = valid ? p : a.n - 1;
  const float om = valid ? a.omega : 0.f;
  const int K = a.K;
  const int64_t nD = a.n * D, pD = pc * D;
  const float* tz = a.keep;
  const float* trho = a.keep + (int64_t)(K + 1) * nD;
  const float* trhop = a.keep + (int64_t)(2 * K + 2) * nD;
  const float* tres = a.keep + (int64_t)(3 * K + 2) * nD;
  const int64_t rowlen = 2 * D + 2 + K;
  float* out = a.gpart + tile * rowlen;
  float qmean[D], qiv[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    qmean[j] = a.params[a.lay.vd_mean + j];
    const float sd = expf(a.params[a.lay.vd_logdiag + j]);
    qiv[j] = 1.0f / (sd * sd);
  }
  const float eps = a.params[a.lay.eps], gamma = a.params[a.lay.gamma];
  const float eta = gamma * eps, ome = 1.0f - eta, i2e = 1.0f / (2.0f * eta);
  constexpr int HN = Target<TARGET, D>::HN;
  float zb[D], rb[D], gmu[D], glam[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    zb[j] = 0.f;
    rb[j] = om * trho[(int64_t)K * nD + pD + j];   // loss += |rho_K|^2 / 2
    gmu[j] = 0.f;
    glam[j] = 0.f;
  }
  float geps = 0.f, geta = 0.f, gb_acc = 0.f;
  for (int m = K; m >= 0; --m) {
    float z[D], gp[D], gq[D], hs[HN], logp;
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = tz[(int64_t)m * nD + pD + j];
    Target<TARGET, D>::eval_hess(z, g, lds_tgt, logp, gp, hs);
#pragma unroll
    for (int j = 0; j < D; ++j) gq[j] = -(z[j] - qmean[j]) * qiv[j];
    float a_gp[D], a_gq[D], vz[D];
#pragma unroll
    for (int j = 0; j < D; ++j) { a_gp[j] = 0.f; a_gq[j] = 0.f; vz[j] = 0.f; }
    if (m < K) {
      const float be = a.ws[a.w.beta + m];
      float sb = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float rhop = trhop[(int64_t)m * nD + pD + j], rhoi = trho[(int64_t)m * nD + pD + j];
        const float res = tres[(int64_t)m * nD + pD + j];
        const float gU = -1.0f * (be * gp[j] + (1.0f - be) * gq[j]);
        const float rpp = rhop - 0.5f * eps * gU;
        // drift z_{m+1} = z_m + eps rho''
        geps += zb[j] * rpp;
        rb[j] += eps * zb[j];
        // opening kick rho'' = rho' - eps/2 gU(z_m, beta_m)
        a_gp[j] += be * 0.5f * eps * rb[j];
        a_gq[j] += (1.0f - be) * 0.5f * eps * rb[j];
        sb += (gp[j] - gq[j]) * rb[j];
        geps -= 0.5f * gU * rb[j];
        // weight term |res|^2 / (4 eta)
        const float gbm = -om * res * i2e;            // d / d m_b
        geta -= om * res * res * i2e * i2e;
        float rpb = rb[j] + ome * gbm;                // d / d rho'
        geta -= rhop * gbm;
        if (NET) {   // (a lane past the batch reads the last particle's row: its cotangent is not this lane's)
          rpb += valid ? a.vin[((int64_t)m * a.n + pc) * (2 * D) + D + j] : 0.f;
          vz[j] = valid ? a.vin[((int64_t)m * a.n + pc) * (2 * D) + j] : 0.f;
          geta += (rhoi - res - ome * rhop) * gbm * 2.0f * i2e;   // 2 s . g_b with s = (m_b - (1 - eta) rho') / (2 eta)
        }
        // refresh rho' = (1 - eta) rho_m + sigma n,  sigma n = rho' - (1 - eta) rho_m,  d sigma / d eta = 1 / sigma
        geta += rpb * (-rhoi + (rhop - ome * rhoi) * i2e);
        rb[j] = ome * rpb - gbm;                      // d / d rho_m
      }
      gb_acc += 0.5f * eps * sb;
      const float tb = row_sum16(gb_acc);
      if (lane == 0) out[2 * D + 2 + m] = tb;
      gb_acc = 0.f;
    }
    if (m > 0) {   // closing kick of bridge m - 1: rho_m = rho'' - eps/2 gU(z_m, beta_{m-1})
      const float bp = a.ws[a.w.beta + m - 1];
      float sb = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float gU = -1.0f * (bp * gp[j] + (1.0f - bp) * gq[j]);
        a_gp[j] += bp * 0.5f * eps * rb[j];
        a_gq[j] += (1.0f - bp) * 0.5f * eps * rb[j];
        sb += (gp[j] - gq[j]) * rb[j];
        geps -= 0.5f * gU * rb[j];
      }
      gb_acc += 0.5f * eps * sb;
    }
    float hv[D];
    Target<TARGET, D>::hvp(hs, z, a_gp, hv);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      if (m == K) zb[j] -= om * gp[j];               // loss -= log p(z_K)
      zb[j] += hv[j] - a_gq[j] * qiv[j] + vz[j];
      gmu[j] += a_gq[j] * qiv[j];
      glam[j] += a_gq[j] * (-2.0f * gq[j]);
      if (m == 0) {   // z_0 = mean + std e,  log q(z_0) = -|e|^2 / 2 - sum logdiag - const
        gmu[j] += zb[j];
        glam[j] += zb[j] * (z[j] - qmean[j]) - om;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float tm = row_sum16(gmu[j]), tl = row_sum16(glam[j]);
    if (lane == 0) {
      out[j] = tm;
      out[D + j] = tl;
    }
  }
  geps += gamma * geta;
  const float te = row_sum16(geps), tg = row_sum16(eps * geta);
  if (lane == 0) {
    out[2 * D] = te;
    out[2 * D + 1] = tg;
  }
}

// ------------------------------------------------------------------------------------------
// fixed-order sums: one thread per output over its `count` terms (eight loads in flight; term t goes to chain t % 8, the chains
// are added in a fixed tree).  Outputs: the slab entries -> grad (true width IN); the per-item rows -> the S / S2 tables of the
// tails; the sweep's per-tile rows -> grad (vd, gamma) and the per-bridge tables {d beta[K], d eps at slot 0}.
// ------------------------------------------------------------------------------------------
struct LdviReduceArgs {
  const float* slabs;
  const float* rows;
  const float* gpart;
  float* grad;
  float* gtab;              // S[K+1][HP] | S2[K+1][HP] | gbeta[al4 K] | geps[al4 K]   (zeroed before this launch)
  cmcd_layout lay;
  int64_t tiles, o_S, o_S2, o_gbeta, o_geps;
  int32_t K, D, HP, IN, nslabs, net;
};

__device__ __forceinline__ float ldvi_sum_terms(const float* base, int64_t stride, int64_t count) {
  float acc[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = 0.f;
  int64_t t = 0;
  for (; t + 8 <= count; t += 8) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = base[(t + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] += x[u];
  }
  for (; t < count; ++t) acc[0] += base[t * stride];
  return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

__global__ __launch_bounds__(256) void ldvi_reduce_kernel(LdviReduceArgs a) {
  const int D = a.D, HP = a.HP, IN = a.IN, K = a.K, TJ16 = 16 * ldvi_tj(D);
  const int64_t slabf = a.net ? ldvi_slab_floats(D, HP) : 0;
  const int64_t n_rows = a.net ? (int64_t)K * 2 * HP : 0;
  const int64_t rowlen = 2 * D + 2 + K;
  const int64_t total = slabf + n_rows + rowlen;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    if (o < slabf) {
      int64_t dst = -1, i = o;
      if (i < (int64_t)HP * HP) {
        const int k = int(i / HP), m = int(i % HP);
        if (k < IN && m < IN) dst = a.lay.g_w2 + (int64_t)k * IN + m;
      } else if ((i -= (int64_t)HP * HP) < (int64_t)TJ16 * HP) {
        const int j = int(i / HP), m = int(i % HP);
        if (j < 2 * D && m < IN) dst = a.lay.g_w1 + (int64_t)j * IN + m;
      } else if ((i -= (int64_t)TJ16 * HP) < (int64_t)HP * 16) {
        const int k = int(i / 16), j = int(i % 16);
        if (k < IN && j < D) dst = a.lay.g_w3 + (int64_t)k * D + j;
      } else if ((i -= (int64_t)HP * 16) < HP) {
        if (i < IN) dst = a.lay.g_b2 + i;
      } else {
        i -= HP;
        if (i < D) dst = a.lay.g_b3 + i;
        else if (i == 15) dst = a.lay.g_factor;
      }
      if (dst >= 0) a.grad[dst] = ldvi_sum_terms(a.slabs + o, slabf, a.nslabs);
    } else if (o - slabf < n_rows) {
      const int64_t q = o - slabf;
      const int i = int(q / (2 * HP)), e = int(q % (2 * HP));
      const float v = ldvi_sum_terms(a.rows + (int64_t)i * a.tiles * 2 * HP + e, 2 * HP, a.tiles);
      a.gtab[(e < HP ? a.o_S : a.o_S2) + (int64_t)i * HP + (e < HP ? e : e - HP)] = v;
    } else {
      const int64_t q = o - slabf - n_rows;
      const float v = ldvi_sum_terms(a.gpart + q, rowlen, a.tiles);
      if (q < D) a.grad[a.lay.vd_mean + q] = v;
      else if (q < 2 * D) a.grad[a.lay.vd_logdiag + (q - D)] = v;
      else if (q == 2 * D) a.gtab[a.o_geps] = v;
      else if (q == 2 * D + 1) a.grad[a.lay.gamma] = v;
      else a.gtab[a.o_gbeta + (q - (2 * D + 2))] = v;
    }
  }
}

// grad[n_grad] and gtab[n_gtab] start from zero.  A launch, not two hipMemsetAsync: captured into a graph those become memset
// nodes, and from the second replay on a gradient call replayed behind other work of its stream returned garbage in the
// entries the zeroed part of gtab feeds (d eps, the last embedding row, b1, W1[2 d:]); kernel nodes replay in order.
__global__ __launch_bounds__(256) void ldvi_zero_kernel(float* grad, int64_t n_grad, float* gtab, int64_t n_gtab) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_grad + n_gtab; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n_grad) grad[i] = 0.f;
    else gtab[i - n_grad] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
typedef void (*ldvi_fn)(LdviArgs);

template <int TARGET, int D>
static ldvi_fn ldvi_traj_pick(int T, bool net) {
  if (!net) return ldvi_traj_kernel<TARGET, D, 1, false>;
  if constexpr (D == 2) {
    if (T == 2) return ldvi_traj_kernel<TARGET, D, 2, true>;
    if (T == 4) return ldvi_traj_kernel<TARGET, D, 4, true>;
  } else {
    if (T == 5) return ldvi_traj_kernel<TARGET, D, 5, true>;
  }
  return nullptr;
}

// gmm / many_gmm (d = 2) on 2 and 4 neuron tiles, the funnel (d = 10) on 5; without a network the same three (target, dim)
static ldvi_fn ldvi_traj_fn(const cmcd_desc& d, int T, bool net) {
  if (net && d.arch != CMCD_ARCH_GEFFNER) return nullptr;
  if (d.target == CMCD_TARGET_GMM && d.dim == 2) return ldvi_traj_pick<CMCD_TARGET_GMM, 2>(T, net);
  if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) return ldvi_traj_pick<CMCD_TARGET_MANY_GMM, 2>(T, net);
  if (d.target == CMCD_TARGET_FUNNEL && d.dim == 10) return ldvi_traj_pick<CMCD_TARGET_FUNNEL, 10>(T, net);
  return nullptr;
}

static ldvi_fn ldvi_item_fn(const cmcd_desc& d, int T) {
  if (d.dim == 2) return T == 2 ? ldvi_net_grad_kernel<2, 2> : (T == 4 ? ldvi_net_grad_kernel<2, 4> : nullptr);
  if (d.dim == 10 && T == 5) return ldvi_net_grad_kernel<10, 5>;
  return nullptr;
}

template <bool NET>
struct LdviSweep {
  typedef ldvi_fn fn;
  template <int TARGET, int D> static fn get() { return ldvi_sweep_kernel<TARGET, D, NET>; }
};

bool ldvi_available(const cmcd_desc& d, int T, bool use_net) { return ldvi_traj_fn(d, T, use_net) != nullptr; }

struct LdviWs {
  int64_t keep, vin, rows, slabs, gpart, gtab, o_S, o_S2, o_gbeta, o_geps, gtab_floats, total;   // floats, from gws
  int32_t nslabs;
};
static LdviWs ldvi_ws(const cmcd_desc& d, int HP, int64_t n, bool net) {
  const int64_t K = d.nbridges, D = d.dim, tiles = (n + 15) / 16, items = K * tiles;
  LdviWs w{};
  w.nslabs = net ? (int32_t)(items < kLdviMaxSlabs ? items : kLdviMaxSlabs) : 0;
  int64_t o = 0;
  w.keep = o; o += al4((4 * K + 2) * n * D);
  w.vin = o; o += net ? al4(K * n * 2 * D) : 0;
  w.rows = o; o += net ? al4(items * 2 * HP) : 0;
  w.slabs = o; o += net ? al4((int64_t)w.nslabs * ldvi_slab_floats((int)D, HP)) : 0;
  w.gpart = o; o += al4(tiles * (2 * D + 2 + K));
  w.gtab = o;
  w.o_S = 0;
  w.o_S2 = w.o_S + (net ? (K + 1) * HP : 0);
  w.o_gbeta = w.o_S2 + (net ? (K + 1) * HP : 0);
  w.o_geps = w.o_gbeta + al4(K);
  w.gtab_floats = w.o_geps + al4(K);
  o += al4(w.gtab_floats);
  w.total = o;
  return w;
}

int64_t ldvi_grad_floats(const cmcd_desc& d, int HP, int64_t n, bool use_net) { return ldvi_ws(d, HP, n, use_net).total; }

int ldvi_launch(const cmcd_desc& d, const cmcd_layout& lay, const WsLayout& w, bool use_net, const int32_t* seeds, int64_t n,
                const float* params, int64_t n_params, float* ws, float* gws, float omega, float* out_loss, float* out_z,
                float* grad, hipStream_t stream) {
  const int D = d.dim, K = d.nbridges, HP = w.HP, T = w.T;
  ldvi_fn traj = ldvi_traj_fn(d, T, use_net);
  if (!traj) return fail(CMCD_ERR_UNSUPPORTED, "no LDVI kernel instance for this (target, dim, arch, width=%s%lld)", "", HP);
  const int64_t tiles = (n + 15) / 16;
  LdviWs g{};
  LdviArgs a{};
  a.seeds = seeds; a.params = params; a.ws = ws; a.partials = reinterpret_cast<double*>(ws + w.partials);
  a.out_loss = out_loss; a.out_z = out_z; a.lay = lay; a.w = w; a.n = n; a.K = K; a.omega = omega;
  if (grad) {
    g = ldvi_ws(d, HP, n, use_net);
    a.keep = gws + g.keep; a.gpart = gws + g.gpart; a.nslabs = g.nslabs;
    if (use_net) { a.vin = gws + g.vin; a.rows = gws + g.rows; a.slabs = gws + g.slabs; }
  }
  {
    const size_t lds_bytes = size_t((use_net ? HP * HP + 3 * D * HP + HP + 16 : 0) + w.tgt_floats) * 4;
    // waves per workgroup: the 2nd-order wave-per-tile kernel's rule (one wave per workgroup until every SIMD has one)
    const int nw = tiles <= 1024 ? 1 : (tiles <= 8192 ? 4 : 8);
    hipLaunchKernelGGL(traj, dim3(unsigned((tiles + nw - 1) / nw)), dim3(64 * nw), lds_bytes, stream, a);
  }
  if (!grad) return hipGetLastError() == hipSuccess ? CMCD_OK : fail(CMCD_ERR_HIP, "LDVI launch failed%s");

  {
    const int64_t zeros = n_params + g.gtab_floats, blocks = (zeros + 255) / 256;
    hipLaunchKernelGGL(ldvi_zero_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream, grad, n_params,
                       gws + g.gtab, g.gtab_floats);
  }
  if (use_net) {
    ldvi_fn item = ldvi_item_fn(d, T);
    if (!item) return fail(CMCD_ERR_UNSUPPORTED, "no LDVI network-gradient instance for this (dim, width=%s%lld)", "", HP);
    const size_t lds_bytes = size_t(16 * ldvi_tj(D) + 4 * HP + 16) * kLdviPad * 4;
    hipLaunchKernelGGL(item, dim3((unsigned)g.nslabs), dim3(64), lds_bytes, stream, a);
  }
  ldvi_fn sweep = use_net ? tile_pick_plain<LdviSweep<true>>(d.target, D) : tile_pick_plain<LdviSweep<false>>(d.target, D);
  hipLaunchKernelGGL(sweep, dim3((unsigned)((tiles + 3) / 4)), dim3(256), size_t(w.tgt_floats) * 4, stream, a);
  LdviReduceArgs ra{};
  ra.slabs = a.slabs; ra.rows = a.rows; ra.gpart = a.gpart; ra.grad = grad; ra.gtab = gws + g.gtab; ra.lay = lay;
  ra.tiles = tiles; ra.o_S = g.o_S; ra.o_S2 = g.o_S2; ra.o_gbeta = g.o_gbeta; ra.o_geps = g.o_geps;
  ra.K = K; ra.D = D; ra.HP = HP; ra.IN = 2 * D + d.emb_dim; ra.nslabs = g.nslabs; ra.net = use_net ? 1 : 0;
  const int64_t outs = (use_net ? ldvi_slab_floats(D, HP) + (int64_t)K * 2 * HP : 0) + 2 * D + 2 + K;
  hipLaunchKernelGGL(ldvi_reduce_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, stream, ra);
  if (hipGetLastError() != hipSuccess) return fail(CMCD_ERR_HIP, "LDVI gradient launch failed%s");
  // d eps and d mgridref_y from the per-bridge tables, then the embedding table, b1 and W1[2 d:] from S / S2 (cmcd_grad.hip)
  cmcd_desc e = d;
  e.eps_schedule = CMCD_EPS_CONST;
  int rc;
  if (use_net)
    rc = launch_net_tails(e, 2 * D, CMCD_EPS_CONST, lay, w, params, gws + g.gtab, g.o_S, g.o_S2, g.o_gbeta, g.o_geps, HP, nullptr,
                          grad, stream);
  else
    rc = launch_geffner_tails(e, lay, w, params, gws + g.gtab, g.o_S, g.o_S2, g.o_gbeta, g.o_geps, HP, grad, stream, false);
  return rc == CMCD_OK ? CMCD_OK : fail(rc, "LDVI tail launch failed%s");
}

}  // namespace cmcd
