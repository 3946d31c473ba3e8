// Resumable segments of the LDVI forward chain (MCD_U_a-lp-sn and its network-free sibling MCD_U_a-lp) on gfx950: bridges
// [k0, k1) from a caller-supplied particle state that carries the momentum, so that the weights can be examined (and the
// particles resampled) between bridges — cmcd_segment_uha.hip for the first of the two momentum baselines.
//
// The reference has no such call; the arithmetic is the forward call's (cmcd_ldvi.hip: ldvi_traj_kernel, reference lines
// mcd_under_lp_a.py:6-87), cut at a bridge, and is written out in include/cmcd_hip.h (cmcd_bound_segment_ldvi).  Per particle,
// with eta = gamma eps, sigma = sqrt(2 eta), gU(z, b) = -(b grad log p(z) + (1 - b) grad log q(z)) (no clip), eps the scalar leaf:
//
//   k0 == 0:  key chain, z_0 and rho_0 exactly as ldvi_traj_kernel;  wpath = -log q(z_0) - log N(rho_0; 0, I);  gen = gen_0
//   k0  > 0:  z, rho, wpath, gen = the caller's state                    (gen: the forward chain's gen_k0)
//   for i = k0 .. k1-1, the forward call's bridge i:
//             m_f = rho (1 - eta);  rho' = m_f + sigma n_i                              (no network; n_i: the deviate of gen_i)
//             rho'' = rho' - eps gU(z, beta_i) / 2;  z' = z + eps rho'';  rho_new = rho'' - eps gU(z', beta_i) / 2
//             m_b = rho' (1 - eta) [+ 2 eta s([z; rho'], i)]                            (old z; the network only when NET)
//             wpath += log N(rho; m_b, sigma) - log N(rho'; m_f, sigma);  gen <- second(split(second(split(gen))))
//   lg = log gamma_k1(z) + log N(rho; 0, I):  gamma_K = p;  0 < k < K: log gamma_k = beta_{k-1} log p + (1 - beta_{k-1}) log q
//                          (log p = -inf — the many_gmm floor — gives lg = -inf, never 0 * inf; a NaN stays a NaN)
//   out: z, rho, wpath, lg, key = gen_k1;  statistics over l := -(wpath + lg)
//
// Segments compose bit for bit — [0, k) then [k, K) returns the bits of [0, K) in z, rho, wpath, lg and the key — by the
// structure of cmcd_segment_uha.hip: ONE runtime-bounded rotated loop, m = k0 .. k1, with a SINGLE site that evaluates
// (log p, grad log p, grad log q) at z_m.  For m > k0 that evaluation closes bridge m - 1 (rho = rho'' - eps ub / 2), for m < k1
// it opens bridge m, at m == k1 it forms lg.  The network evaluation of a bridge needs the bridge's own rho' and stays inside
// the bridge, at one site.  At a cut both segments run the same machine code on the same (z_k, rho''): one extra target
// evaluation per cut.
//
// Mapping = ldvi_traj_kernel's (cmcd_tile.h): one wave per 16-particle tile, lane (g, c) = particle c; layer 2 on
// v_mfma_f32_16x16x4_f32 from the packed W2 fragments in LDS (cmcd_mom.h); z, rho, wpath and the key in registers; one
// statistics record per tile for finalize_kernel.  Plain vector stores only.
#include "cmcd_mom.h"

namespace cmcd {

struct SegmentLdviArgs {
  const int32_t* seeds;     // read when k0 == 0
  const float* params;
  const float* ws;          // the prep launch's tables
  double* partials;         // [tiles][5]
  float* z;                 // [n][D]  in (k0 > 0) and out
  float* rho;               // [n][D]  in (k0 > 0) and out
  float* wpath;             // [n]     in (k0 > 0) and out
  uint32_t* key;            // [n][2]  in (k0 > 0) and out: gen_k0 -> gen_k1
  float* lg;                // [n]     out
  cmcd_layout lay;
  WsLayout w;
  int64_t n;
  int32_t K, k0, k1;        // bridges [k0, k1), 0 <= k0 < k1 <= K
};

// term j of log q(z) for q = N(mean, exp(logdiag)^2), the standard deviation formed from the parameters where it is needed (the
// start of the chain and lg): carried over the loop the D of them would sit in registers that no bridge reads
__device__ __forceinline__ float seg_ldvi_log_q_term(float zj, float mean, const float* params, int64_t off) {
  float ld = params[off];
  asm volatile("" : "+v"(ld));
  const float sd = expf(ld);
  const float dz = zj - mean;
  return -(dz * dz) / (2.0f * sd * sd) - logf(sd) - kHalfLog2Pi;
}

// Dynamic LDS, ldvi_traj_kernel's: NET: w2 | w1z[2 D] | w3t | b2 | b3[16] | target constants; without a network the constants alone.
template <int TARGET, int D, int T, bool NET>
__global__ __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4) void segment_ldvi_kernel(SegmentLdviArgs a) {
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
  const int ks = a.k0, ke = a.k1, K = a.K;

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

  uint32_t k0, k1;
  float z[D], rho[D];
  float w;
  if (ks == 0) {
    // ---- the forward call's start (mcdboundingmachine.py:151-162; mcd_under_lp_a.py:66-67,74):
    // (A, B) = split(PRNGKey(seed)); z_0 = mean + std normal(A); C = first(split(B)); (R, G') = split(C); rho_0 = normal(R);
    // gen_0 = second(split(G'))
    const int gb = g & 1;
    const int32_t seed = a.seeds[pl];
    uint32_t x0, x1;
    tile_split(0u, (uint32_t)seed, gb, x0, x1);
    uint32_t a0, a1, b0, b1;
    rows01(x0, a0, a1);
    rows01(x1, b0, b1);
    float nz[2 * Hh];
    tile_normal<D>(a0, a1, g, nz);
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = expf(a.params[a.lay.vd_logdiag + j]) * nz[j] + qmean[j];
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
    for (int j = 0; j < D; ++j) w -= seg_ldvi_log_q_term(z[j], qmean[j], a.params, a.lay.vd_logdiag + j);
    w -= mom_log_n01<D>(rho);
  } else {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      z[j] = a.z[pl * D + j];
      rho[j] = a.rho[pl * D + j];
    }
    w = a.wpath[pl];
    k0 = a.key[pl * 2];
    k1 = a.key[pl * 2 + 1];
  }

  const float* bias1 = a.ws + a.w.bias1;
  const float* utab = a.ws + a.w.utab;

  // Rotated loop over the states z_k0 .. z_k1: iteration m evaluates log p, grad log p and grad log q ONCE, at z_m.
  // `rho` holds rho_m once bridge m - 1 is closed, and rho'' of bridge m from the bridge's end to the top of the next iteration.
  float pbeta = 0.f;                 // beta_{m-1} (set when bridge m - 1 was opened)
  float logp = 0.f;

  for (int m = ks; m <= ke; ++m) {
    float gp[D], gq[D];
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
#pragma unroll
    for (int j = 0; j < D; ++j) gq[j] = -(z[j] - qmean[j]) * qiv[j];

    if (m > ks) {
      // ---- second half-kick of bridge m - 1 at z_m: closes the bridge
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float ub = -1.0f * (pbeta * gp[j] + (1.0f - pbeta) * gq[j]);   // (beta_{m-1})
        rho[j] = rho[j] - eps * ub / 2.0f;                                   // :37
      }
    }
    if (m == ke) break;

    // ---- bridge m: the momentum refresh (no network), the backward kernel's mean (the network), both densities, the first
    // half-kick and the drift
    const float beta = mom_uniform(a.ws[a.w.beta + m]);
    float nz[2 * Hh];
    tile_chain_step<D>(k0, k1, g, nz);                // (G, H) = split(gen); n_m = normal(G); gen = second(split(H))
    // the half-kick is formed here so that grad log p and grad log q are not carried over the network evaluation
    float hk[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float uf = -1.0f * (beta * gp[j] + (1.0f - beta) * gq[j]);
      hk[j] = eps * uf / 2.0f;
    }
    float rhop[D], s[D];
    float fk_lp = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float mf = rho[j] * ome;                   // :29
      rhop[j] = mf + sig * nz[j];                      // :33
      const float df = rhop[j] - mf;
      fk_lp += -(df * df) * inv2s2 - cst;              // log N(rho'; m_f, sigma)   :54
      s[j] = 0.f;
    }
    if (NET) {
      f32x4 prez[T];
      mom_pre_z<D, T>(z, bias1 + (int64_t)m * HP, lds_w1z, g, prez);
      mom_eval_rho<D, T>(prez, z, rhop, utab + (int64_t)m * HP, lds_w2, lds_w1z, lds_b2, lds_w3t, lds_b3, lane, s);
    }
    float bk_lp = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float mb = NET ? rhop[j] * ome + 2.0f * eta * s[j] : rhop[j] * ome;   // :41-51
      const float db = rho[j] - mb;
      bk_lp += -(db * db) * inv2s2 - cst;              // log N(rho; m_b, sigma)    :55
      rho[j] = rhop[j] - hk[j];                        // :35   rho''
      z[j] = z[j] + eps * rho[j];                      // :36
    }
    w += bk_lp - fk_lp;                                // :58
    pbeta = beta;
  }

  // lg = log gamma_k1(z_k1) + log N(rho_k1; 0, I): log p at the end of the chain, the geometric bridge of bridge k1 - 1 before it
  float lg = logp;
  if (ke < K) {
    float logq = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) logq += seg_ldvi_log_q_term(z[j], qmean[j], a.params, a.lay.vd_logdiag + j);
    const float bl = a.ws[a.w.beta + (ke - 1)];
    lg = (logp == -INFINITY) ? -INFINITY : bl * logp + (1.0f - bl) * logq;
  }
  lg += mom_log_n01<D>(rho);     // (-inf stays -inf: the momentum term is never +inf; a NaN momentum gives NaN)
  const float loss = -(w + lg);

  if (valid && g == 0) {
    a.wpath[p] = w;
    a.lg[p] = lg;
    a.key[p * 2] = k0;
    a.key[p * 2 + 1] = k1;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      a.z[p * D + j] = z[j];
      a.rho[p * D + j] = rho[j];
    }
  }

  tile_stats_record(loss, valid && g == 0, lane, a.partials + tile * CMCD_NSTATS);
}

// ------------------------------------------------------------------------------------------
// launcher (cmcd_host.h): the instance table of cmcd_ldvi.hip's ldvi_traj_pick, the launch rule of ldvi_launch
// ------------------------------------------------------------------------------------------
typedef void (*segment_ldvi_fn)(SegmentLdviArgs);

template <int TARGET, int D>
static segment_ldvi_fn segment_ldvi_pick(int T, bool net) {
  if (!net) return segment_ldvi_kernel<TARGET, D, 1, false>;
  if constexpr (D == 2) {
    if (T == 2) return segment_ldvi_kernel<TARGET, D, 2, true>;
    if (T == 4) return segment_ldvi_kernel<TARGET, D, 4, true>;
  } else {
    if (T == 5) return segment_ldvi_kernel<TARGET, D, 5, true>;
  }
  return nullptr;
}

// gmm / many_gmm (d = 2) on 2 and 4 neuron tiles, the funnel (d = 10) on 5; without a network the same three (target, dim)
static segment_ldvi_fn segment_ldvi_fn_of(const cmcd_desc& d, int T, bool net) {
  if (net && d.arch != CMCD_ARCH_GEFFNER) return nullptr;
  if (d.target == CMCD_TARGET_GMM && d.dim == 2) return segment_ldvi_pick<CMCD_TARGET_GMM, 2>(T, net);
  if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) return segment_ldvi_pick<CMCD_TARGET_MANY_GMM, 2>(T, net);
  if (d.target == CMCD_TARGET_FUNNEL && d.dim == 10) return segment_ldvi_pick<CMCD_TARGET_FUNNEL, 10>(T, net);
  return nullptr;
}

bool segment_ldvi_available(const cmcd_desc& d, int T, bool use_net) { return segment_ldvi_fn_of(d, T, use_net) != nullptr; }

int segment_ldvi_launch(const cmcd_desc& d, const cmcd_layout& lay, const WsLayout& w, bool use_net, int32_t k0, int32_t k1,
                        const int32_t* seeds, int64_t n, const float* params, float* ws, float* z, float* rho, float* wpath,
                        uint32_t* key, float* lg, hipStream_t stream) {
  const int D = d.dim, HP = w.HP;
  segment_ldvi_fn fn = segment_ldvi_fn_of(d, w.T, use_net);
  if (!fn) return fail(CMCD_ERR_UNSUPPORTED, "no LDVI segment kernel instance for this (target, dim, arch, width=%s%lld)", "", HP);
  const int64_t tiles = (n + 15) / 16;
  SegmentLdviArgs a{seeds, params, ws, reinterpret_cast<double*>(ws + w.partials), z, rho, wpath, key, lg, lay, w, n,
                    (int32_t)d.nbridges, k0, k1};
  const size_t lds_bytes = size_t((use_net ? HP * HP + 3 * D * HP + HP + 16 : 0) + w.tgt_floats) * 4;
  // waves per workgroup: ldvi_launch's rule (one wave per workgroup until every SIMD has one)
  const int nw = tiles <= 1024 ? 1 : (tiles <= 8192 ? 4 : 8);
  hipLaunchKernelGGL(fn, dim3(unsigned((tiles + nw - 1) / nw)), dim3(64 * nw), lds_bytes, stream, a);
  return hipGetLastError() == hipSuccess ? CMCD_OK : fail(CMCD_ERR_HIP, "LDVI segment launch failed%s");
}

}  // namespace cmcd
