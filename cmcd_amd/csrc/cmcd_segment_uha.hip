// Resumable segments of the 2nd-order (underdamped) forward chain, MCD_CAIS_UHA_sn, on gfx950: bridges [k0, k1) from a
// caller-supplied particle state that carries the momentum, so that the weights can be examined (and the particles resampled)
// between bridges — sequential Monte Carlo over the annealing path for the mode cmcd_segment.hip has no kernel for.
//
// The reference has no such call; the arithmetic is the forward call's (cmcd_uha.hip: uha_traj_kernel, reference lines
// mcd_under_lp_a_cais.py:41-113), cut at a bridge, and is written out in include/cmcd_hip.h (cmcd_bound_segment_uha).  Per
// particle, with the schedules beta_i, eps_i (cos^2), the clip of grad log p at 1e2, the network s([z; rho], i) and q of
// cmcd_bound_forward in this mode (the same prep tables), eta = gamma eps_i, sigma = sqrt(2 eta):
//
//   k0 == 0:  key chain, z_0 and rho_0 exactly as uha_traj_kernel;  wpath = -log q(z_0) - log N(rho_0; 0, I);  gen = gen_0
//   k0  > 0:  z, rho, wpath, gen = the caller's state                    (gen: the forward chain's gen_k0)
//   for i = k0 .. k1-1, the forward call's bridge i:
//             m_f = rho (1 - eta) - 2 eta s([z; rho], i);  rho' = m_f + sigma n_i         (n_i: the deviate of gen_i)
//             rho'' = rho' - eps uf / 2;  z' = z + eps rho'';  rho_new = rho'' - eps ub(z') / 2          (leap-frog, beta_i at both ends)
//             m_b = rho' (1 - eta) + 2 eta s([z; rho'], i)                                 (old z, same index i)
//             wpath += log N(rho; m_b, sigma) - log N(rho'; m_f, sigma);  gen <- second(split(second(split(gen))))
//   lg = log gamma_k1(z) + log N(rho; 0, I):  gamma_K = p;  0 < k < K: log gamma_k = beta_{k-1} log p + (1 - beta_{k-1}) log q
//                          (log p = -inf — the many_gmm floor — gives lg = -inf, never 0 * inf; a NaN stays a NaN)
//   out: z, rho, wpath, lg, key = gen_k1;  statistics over l := -(wpath + lg)
//
// Segments compose bit for bit — [0, k) then [k, K) returns the bits of [0, K) in z, rho, wpath, lg and the key — by structure:
// ONE runtime-bounded rotated loop, m = k0 .. k1, with a SINGLE site that evaluates (log p, grad log p, grad log q) at z_m.  For
// m > k0 that evaluation closes step m - 1 (rho = rho'' - eps_{m-1} ub / 2), for m < k1 it opens step m, at m == k1 it forms lg.
// The two network evaluations of a step need the step's own momenta and stay inside the step, at the same two sites in every
// iteration.  At a cut both segments run the same machine code on the same (z_k, rho''): one extra target evaluation per cut.
//
// Mapping = uha_traj_kernel's: one wave owns 16 particles for the whole segment, lane (g, c) holds particle c and the hidden units
// {16 t + 4 g + r}; layer 2 on v_mfma_f32_16x16x4_f32 with the packed W2 A fragments streamed from LDS, layers 1 and 3 on the
// VALU; z, rho, wpath and the key stay in registers; one statistics record per tile for finalize_kernel.  seg_pre_z /
// seg_eval_rho are COPIES of cmcd_uha.hip's net_pre_z / net_eval_rho, as cmcd_ldvi.hip's are: that file is hashed for the stored
// counter figures (bench.py: kernel_sources_sha) and cannot hand them out through a header.  The key-chain step, the draw, the
// split and the statistics record are cmcd_tile.h's.  Plain vector stores only.
#include "cmcd_tile.h"

namespace cmcd {

struct SegmentUhaArgs {
  TrajArgs t;        // seeds (read when k0 == 0), params, ws, partials, lay, w, n, K; the rest unused
  int32_t k0, k1;    // bridges [k0, k1), 0 <= k0 < k1 <= K
  float* z;          // [n][D]  in (k0 > 0) and out
  float* rho;        // [n][D]  in (k0 > 0) and out
  float* wpath;      // [n]     in (k0 > 0) and out
  uint32_t* key;     // [n][2]  in (k0 > 0) and out: gen_k0 -> gen_k1
  float* lg;         // [n]     out
};

// first-layer pre-activation shared by the two evaluations of a bridge: bias row (time path folded by the prep launch) + z W1[:d]
// (cmcd_uha.hip: net_pre_z)
template <int D, int T>
__device__ __forceinline__ void seg_pre_z(const float (&z)[D], const float* __restrict__ brow, const float* lds_w1z, int g,
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
__device__ __forceinline__ void seg_eval_rho(const f32x4 (&prez)[T], const float (&z)[D], const float (&rho)[D],
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

template <int TARGET, int ARCH, int D, int T>
__global__ __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4) void segment_uha_kernel(SegmentUhaArgs sa) {
  const TrajArgs& a = sa.t;
  constexpr int HP = 16 * T;
  constexpr int Hh = (D + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lds_w2 = lds;                     // HP*HP
  float* lds_w1z = lds_w2 + HP * HP;       // 2D*HP   rows [0, D) = z part, [D, 2D) = rho part
  float* lds_w3t = lds_w1z + 2 * D * HP;   // D*HP
  float* lds_b2 = lds_w3t + D * HP;        // HP
  float* lds_b3 = lds_b2 + HP;             // 16
  float* lds_tgt = lds_b3 + 16;            // tgt_floats
  const int ks = sa.k0, ke = sa.k1, K = a.K;
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
  float qmean[D], qstd[D], qiv[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    qmean[j] = a.params[a.lay.vd_mean + j];
    qstd[j] = expf(a.params[a.lay.vd_logdiag + j]);
    qiv[j] = 1.0f / (qstd[j] * qstd[j]);
  }
  const float gamma = a.params[a.lay.gamma];

  const int gb = g & 1;
  uint32_t k0, k1;
  float z[D], rho[D];
  float w;
  if (ks == 0) {
    // ---- the forward call's start (mcdboundingmachine.py:151-162; mcd_under_lp_a_cais.py:92-93,100):
    // (A, B) = split(PRNGKey(seed)); z_0 = mean + std normal(A); C = first(split(B)); (R, G') = split(C); rho_0 = normal(R);
    // gen_0 = second(split(G'))
    const int32_t seed = a.seeds[pl];
    uint32_t x0, x1;
    tile_split(0u, (uint32_t)seed, gb, x0, x1);
    uint32_t a0, a1, b0, b1;
    rows01(x0, a0, a1);
    rows01(x1, b0, b1);
    float nz[2 * Hh];
    tile_normal<D>(a0, a1, g, nz);
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = qstd[j] * nz[j] + qmean[j];
    tile_split(b0, b1, gb, x0, x1);
    uint32_t c0, c1;
    rows01(x0, c0, c1);
    tile_split(c0, c1, gb, x0, x1);
    uint32_t r0, r1, p0, p1;
    rows01(x0, r0, r1);
    rows01(x1, p0, p1);
    tile_normal<D>(r0, r1, g, nz);
#pragma unroll
    for (int j = 0; j < D; ++j) rho[j] = nz[j];
    tile_split(p0, p1, gb, x0, x1);
    rows01(x1, k0, k1);
    // wpath = -log q(z_0) - log N(rho_0; 0, I)
    w = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float dz = z[j] - qmean[j];
      w -= -(dz * dz) / (2.0f * qstd[j] * qstd[j]) - logf(qstd[j]) - kHalfLog2Pi;
    }
    float l0 = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) l0 += -(rho[j] * rho[j]) * 0.5f - kHalfLog2Pi;
    w -= l0;
  } else {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      z[j] = sa.z[pl * D + j];
      rho[j] = sa.rho[pl * D + j];
    }
    w = sa.wpath[pl];
    k0 = sa.key[pl * 2];
    k1 = sa.key[pl * 2 + 1];
  }

  const float* bias1 = a.ws + a.w.bias1;
  const float* utab = a.ws + a.w.utab;
  constexpr float clipv = 1e2f;   // gradU(z, beta, clip=1e2), stable=True      mcd_under_lp_a_cais.py:23-30,42,46

  // Rotated loop over the states z_k0 .. z_k1: iteration m evaluates log p, grad log p and grad log q ONCE, at z_m.
  float rpp[D];                      // rho'' of step m - 1
  float pbeta = 0.f, peps = 0.f;     // schedule row m - 1 (set when step m - 1 was opened)
  float logp = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) rpp[j] = 0.f;

  for (int m = ks; m <= ke; ++m) {
    float gp[D], gq[D];
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      gp[j] = fminf(fmaxf(gp[j], -clipv), clipv);
      gq[j] = -(z[j] - qmean[j]) * qiv[j];
    }

    if (m > ks) {
      // ---- second half-kick of step m - 1 at z_m: closes the step
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float ub = -1.0f * (pbeta * gp[j] + (1.0f - pbeta) * gq[j]);   // :65 (beta_{m-1})
        rho[j] = rpp[j] - peps * ub / 2.0f;                                  // :67
      }
    }
    if (m == ke) break;

    // ---- step m: momentum refresh, both kernels' densities, first half-kick and drift
    const float beta = a.ws[a.w.beta + m], eps = a.ws[a.w.eps + m];
    const float eta = gamma * eps;                    // :50
    const float sig = sqrtf(2.0f * eta);              // :56
    const float inv2s2 = 1.0f / (2.0f * sig * sig), cst = logf(sig) + kHalfLog2Pi;
    const float ome = 1.0f - eta;
    float nz[2 * Hh];
    tile_chain_step<D>(k0, k1, g, nz);                // (G, H) = split(gen); n_m = normal(G); gen = second(split(H))   :55,84

    f32x4 prez[T];
    seg_pre_z<D, T>(z, bias1 + (int64_t)m * HP, lds_w1z, g, prez);
    float s1[D], s2[D], rhop[D];
    seg_eval_rho<ARCH, D, T>(prez, z, rho, utab + (int64_t)m * HP, lds_w2, lds_w1z, lds_b2, lds_w3t, lds_b3, lane, s1);
    float fk_lp = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float mf = rho[j] * ome - 2.0f * eta * s1[j];           // :52-54
      rhop[j] = mf + sig * nz[j];                                   // :58-59
      const float df = rhop[j] - mf;
      fk_lp += -(df * df) * inv2s2 - cst;                           // log N(rho'; m_f, sigma)   :83
    }
    seg_eval_rho<ARCH, D, T>(prez, z, rhop, utab + (int64_t)m * HP, lds_w2, lds_w1z, lds_b2, lds_w3t, lds_b3, lane, s2);
    float bk_lp = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float mb = rhop[j] * ome + 2.0f * eta * s2[j];          // :77-80
      const float db = rho[j] - mb;
      bk_lp += -(db * db) * inv2s2 - cst;                           // log N(rho; m_b, sigma)    :84
      const float uf = -1.0f * (beta * gp[j] + (1.0f - beta) * gq[j]);
      rpp[j] = rhop[j] - eps * uf / 2.0f;                           // :62
      z[j] = z[j] + eps * rpp[j];                                   // :63
    }
    w += bk_lp - fk_lp;                                             // :88
    pbeta = beta; peps = eps;
  }

  // lg = log gamma_k1(z_k1) + log N(rho_k1; 0, I): log p at the end of the chain, the geometric bridge of step k1 - 1 before it
  float lg = logp;
  if (ke < K) {
    float logq = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float dz = z[j] - qmean[j];
      logq += -(dz * dz) / (2.0f * qstd[j] * qstd[j]) - logf(qstd[j]) - kHalfLog2Pi;
    }
    const float bl = a.ws[a.w.beta + (ke - 1)];
    lg = (logp == -INFINITY) ? -INFINITY : bl * logp + (1.0f - bl) * logq;
  }
  {
    float lN = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) lN += -(rho[j] * rho[j]) * 0.5f - kHalfLog2Pi;
    lg += lN;     // (-inf stays -inf: lN is never +inf; a NaN momentum gives NaN)
  }
  const float loss = -(w + lg);

  if (valid && g == 0) {
    sa.wpath[p] = w;
    sa.lg[p] = lg;
    sa.key[p * 2] = k0;
    sa.key[p * 2 + 1] = k1;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      sa.z[p * D + j] = z[j];
      sa.rho[p * D + j] = rho[j];
    }
  }

  tile_stats_record(loss, valid && g == 0, lane, a.partials + wave * CMCD_NSTATS);
}

// ------------------------------------------------------------------------------------------
// launcher (cmcd_host.h): the instances of the forward call's wave-per-tile 2nd-order kernel (cmcd_uha.hip: uha_pick)
// ------------------------------------------------------------------------------------------
typedef void (*segment_uha_fn)(SegmentUhaArgs);

template <int TARGET, int ARCH, int D>
static segment_uha_fn segment_uha_pick_T(int T) {
  switch (T) {
    case 2: return segment_uha_kernel<TARGET, ARCH, D, 2>;
    case 4: return segment_uha_kernel<TARGET, ARCH, D, 4>;
    case 5: return segment_uha_kernel<TARGET, ARCH, D, 5>;
    case 9: return segment_uha_kernel<TARGET, ARCH, D, 9>;
    default: return nullptr;
  }
}

static segment_uha_fn segment_uha_pick(const cmcd_desc& d, int T) {
  if (d.mode != CMCD_MODE_CAIS_UHA_SN) return nullptr;
  if (d.arch == CMCD_ARCH_DDS) {
    if (T != 4) return nullptr;
    if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) return segment_uha_kernel<CMCD_TARGET_MANY_GMM, CMCD_ARCH_DDS, 2, 4>;
    if (d.target == CMCD_TARGET_GMM && d.dim == 2) return segment_uha_kernel<CMCD_TARGET_GMM, CMCD_ARCH_DDS, 2, 4>;
    if (d.target == CMCD_TARGET_FUNNEL && d.dim == 10) return segment_uha_kernel<CMCD_TARGET_FUNNEL, CMCD_ARCH_DDS, 10, 4>;
    return nullptr;
  }
  if (d.arch != CMCD_ARCH_GEFFNER) return nullptr;
  if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) return segment_uha_pick_T<CMCD_TARGET_MANY_GMM, CMCD_ARCH_GEFFNER, 2>(T);
  if (d.target == CMCD_TARGET_GMM && d.dim == 2) return segment_uha_pick_T<CMCD_TARGET_GMM, CMCD_ARCH_GEFFNER, 2>(T);
  if (d.target == CMCD_TARGET_FUNNEL && d.dim == 10) return segment_uha_pick_T<CMCD_TARGET_FUNNEL, CMCD_ARCH_GEFFNER, 10>(T);
  return nullptr;
}

bool segment_uha_available(const cmcd_desc& d, int T) { return segment_uha_pick(d, T) != nullptr; }

int segment_uha_launch(const cmcd_desc& d, const WsLayout& w, const TrajArgs& ta, int32_t k0, int32_t k1, float* z, float* rho,
                       float* wpath, uint32_t* key, float* lg, hipStream_t stream) {
  segment_uha_fn fn = segment_uha_pick(d, w.T);
  if (!fn) return fail(CMCD_ERR_UNSUPPORTED, "no 2nd-order segment kernel instance for this (mode, target, dim, arch, width=%s%lld)", "", w.HP);
  const int64_t tiles = w.n_waves, D = d.dim;
  // W1 has 2 D input rows ([z; rho]): one more D * HP block than tile_launch sizes for
  const size_t lds_bytes = size_t(w.HP * w.HP + 3 * D * w.HP + w.HP + 16 + w.tgt_floats) * 4;
  if (lds_bytes > 160 * 1024) return fail(CMCD_ERR_UNSUPPORTED, "network too wide for LDS%s");
  // waves per workgroup: tile_launch's rule (= the forward wave-per-tile kernels')
  const int64_t per_cu = (160 * 1024) / (int64_t)lds_bytes;
  int nw = tiles <= 1024 ? 1 : (tiles <= 8192 ? 4 : 8);
  if (per_cu < 2 && tiles > 256) nw = tiles <= 1024 ? 4 : 8;
  CMCD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds_bytes));
  const unsigned blocks = unsigned((tiles + nw - 1) / nw);
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64 * nw), lds_bytes, stream, SegmentUhaArgs{ta, k0, k1, z, rho, wpath, key, lg});
  return CMCD_OK;
}

}  // namespace cmcd
