// The reverse-time chain of the overdamped modes on gfx950: target draws pushed through the BACKWARD kernels of the sampler.
//
// The reference has no such call (it runs its chain from q only); what is restated here is the arithmetic of its forward
// chain, walked the other way.  Per particle, with the schedules beta_i, eps_i, the clip rule, the network s(., i) and q of
// the forward call (/root/reference/src/mcd_cais.py:24-30,34-44,46-89; mcd_cais_var.py:33-40; mcd_over_orig.py:22-56;
// mcdboundingmachine.py:126-179) and sigma_i = sqrt(2 eps_i):
//
//   z_K = x;  w = log p(z_K)                                                        mcdboundingmachine.py:178
//   for i = K-1 .. 0:
//     ub  = gradU(z_{i+1}, beta_i)                                                  mcd_cais.py:71
//     m_b = z_{i+1} - eps_i ub + eps_i s(z_{i+1}, j)                                :73-79   j = i + 1 (CAIS modes), j = i (MCD_ULA_sn,
//                                                                                   mcd_over_orig.py), no network term (MCD_ULA)
//     z_i = m_b + sigma_i xi_r,  r = K-1-i                                          (the draw the forward chain takes from F_i, :67)
//     uf  = gradU(z_i, beta_i)                                                      :52
//     m_f = z_i - eps_i uf - eps_i s(z_i, i)                                        :61      (network term: CAIS modes only)
//     w  += log N(z_i; m_b, sigma_i) - log N(z_{i+1}; m_f, sigma_i)                 :82-86
//   w -= log q(z_0)                                                                 mcdboundingmachine.py:157
//
// i.e. the functional the forward call returns as -loss, on a path drawn from p(z_K) prod B_i instead of q(z_0) prod F_i:
// E[w] >= ln Z (the EUBO), and exp(-w) are the importance weights of the reverse estimate of 1 / Z.
//
// Key chain = the forward call's (mcdboundingmachine.py:151-162, mcd_cais.py:66,87,94) without its first key:
// (_, gen) = split(PRNGKey(seed)); (C, _) = split(gen); gen_0 = second(split(C)); reverse step r: (G, H) = split(gen),
// xi_r = normal(G, (d,)), gen = second(split(H)).
//
// Mapping = the wave-per-tile trajectory kernel's (cmcd_kernels.hip, cmcd_uha.hip; the network, the key-chain step, the statistics
// butterflies, the instance table and the launch are shared with cmcd_segment.hip: cmcd_tile.h): one wave owns 16 particles for all K steps,
// lane (g, c) holds particle c and the hidden units {16 t + 4 g + r}; layer 2 on v_mfma_f32_16x16x4_f32 with the packed W2
// A fragments streamed from LDS, layers 1 and 3 on the VALU from the w1z / w3t tables, the per-bridge bias row (and the geffner
// residual row) from the prep tables.  The loop is rotated like the forward kernel's: the evaluation at (z_m, m) — grad log p,
// grad log q, s(z_m, m) — closes step m (its forward density) and opens step m - 1 (its backward draw): K + 1 evaluations.
// A particle whose x row holds a non-finite entry, or whose w comes out NaN, leaves with w = +inf (weight 0).
#include "cmcd_tile.h"

namespace cmcd {

struct ReverseArgs {
  TrajArgs t;       // out_loss = out_w, out_z = out_z0; traj / fin_* / dbg_* unused
  const float* x;   // [n][D] target draws
};

template <int TARGET, int ARCH, int D, int T>
__global__ __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4) void reverse_traj_kernel(ReverseArgs ra) {
  const TrajArgs& a = ra.t;
  constexpr int HP = 16 * T;
  constexpr int Hh = (D + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lds_w2 = lds;                    // HP*HP
  float* lds_w1z = lds_w2 + HP * HP;      // D*HP
  float* lds_w3t = lds_w1z + D * HP;      // D*HP
  float* lds_b2 = lds_w3t + D * HP;       // HP
  float* lds_b3 = lds_b2 + HP;            // 16
  float* lds_tgt = lds_b3 + 16;           // tgt_floats
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(a.ws + a.w.w1z);
    f32x4* dst = reinterpret_cast<f32x4*>(lds_w1z);
    for (int i = threadIdx.x; i < D * HP / 4; i += blockDim.x) dst[i] = src[i];
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
    const int64_t t1 = (ARCH == CMCD_ARCH_GEFFNER ? a.w.utab : a.w.bias1) + (int64_t)(a.K + 1) * HP;
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
  const int32_t seed = a.seeds[pl];
  const int K = a.K;

  // q = N(mean, exp(logdiag)^2)                          vardist/diag_gauss.py:15-33
  float qmean[D], qstd[D], qiv[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    qmean[j] = a.params[a.lay.vd_mean + j];
    qstd[j] = expf(a.params[a.lay.vd_logdiag + j]);
    qiv[j] = 1.0f / (qstd[j] * qstd[j]);
  }

  // z_K = x
  float z[D];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    z[j] = ra.x[pl * D + j];
    bad = bad || !isfinite(z[j]);
  }

  // ---- key chain: gen_0 = second(split(first(split(second(split(PRNGKey(seed)))))))
  const int gb = g & 1;
  uint32_t k0, k1;
  {
    uint32_t x0, x1;
    tile_split(0u, (uint32_t)seed, gb, x0, x1);   // split(PRNGKey(seed)) -> (A, B); A (the forward call's z_0 key) is not used
    uint32_t b0, b1;
    rows01(x1, b0, b1);
    tile_split(b0, b1, gb, x0, x1);               // C = first(split(B))
    uint32_t c0, c1;
    rows01(x0, c0, c1);
    tile_split(c0, c1, gb, x0, x1);               // gen_0 = second(split(C))          mcd_cais.py:94
    rows01(x1, k0, k1);
  }

  const float clipv = a.var_mode ? 1e2f : 1e3f;  // mcd_cais.py:24 / mcd_cais_var.py:33
  const bool clip_p = a.grad_clipping != 0;
  const bool clip_q = clip_p && a.var_mode;
  const float fsn = a.ula ? 0.f : 1.f;           // the ULA forward kernel has no network term
  const float* bias1 = a.ws + a.w.bias1;
  const float* utab = a.ws + a.w.utab;

  // Rotated loop over the states z_K .. z_0: iteration m evaluates grad log p, grad log q and the network ONCE at z_m.
  float zn[D];           // z_{m+1}
  float bk_lp = 0.f;     // log B_m(z_m | z_{m+1})
  float pbeta = 0.f, peps = 0.f, pinv2s2 = 0.f, pcst = 0.f;   // schedule row m (set when step m was opened)
  float w = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) zn[j] = 0.f;

  for (int m = K; m >= 0; --m) {
    float gp[D], sn[D], logp;
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
    if (m == K) w = logp;   // log p(z_K)
    // CAIS: s(z_m, m) serves the backward mean of step m - 1 and the forward mean of step m;
    // MCD_ULA_sn: s(z_m, m - 1) serves the backward mean of step m - 1 only
    if (a.ula == 1 || (a.ula == 2 && m == 0)) {
#pragma unroll
      for (int j = 0; j < D; ++j) sn[j] = 0.f;
    } else {
      const int64_t row = (a.ula == 2) ? m - 1 : m;
      tile_eval_net<ARCH, D, T, tile_pf(ARCH, D, T), true>(z, bias1 + row * HP, utab + row * HP, lds_w2, lds_w1z, lds_b2,
                                                      lds_w3t, lds_b3, lane, sn);
    }
    float gq[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      gq[j] = -(z[j] - qmean[j]) * qiv[j];
      if (clip_p) gp[j] = fminf(fmaxf(gp[j], -clipv), clipv);
      if (clip_q) gq[j] = fminf(fmaxf(gq[j], -clipv), clipv);
    }

    if (m < K) {
      // ---- forward density of step m: log N(z_{m+1}; m_f(z_m), sigma_m)       mcd_cais.py:52-61,82
      float fk_lp = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float uf = -1.0f * (pbeta * gp[j] + (1.0f - pbeta) * gq[j]);
        const float fk = z[j] - peps * uf - peps * (fsn * sn[j]);
        const float df = zn[j] - fk;
        fk_lp += -(df * df) * pinv2s2 - pcst;
      }
      w += bk_lp - fk_lp;                                                         // :86
    }
    if (m == 0) break;

    // ---- backward draw of step m - 1: z_{m-1} = m_b(z_m) + sigma_{m-1} xi      mcd_cais.py:71-79,83
    const float* scr = a.ws + a.w.sched + 8 * (int64_t)(m - 1);   // {beta, eps, sigma, log sigma + log sqrt(2 pi), 1 / (2 sigma^2), ..}
    const float beta = scr[0], eps = scr[1], sig = scr[2], cst = scr[3], inv2s2 = scr[4];
    float nz[2 * Hh];
    tile_chain_step<D>(k0, k1, g, nz);
    bk_lp = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float ub = -1.0f * (beta * gp[j] + (1.0f - beta) * gq[j]);
      const float bk = z[j] - eps * ub + eps * sn[j];
      const float zo = bk + sig * nz[j];
      const float db = zo - bk;
      bk_lp += -(db * db) * inv2s2 - cst;
      zn[j] = z[j];
      z[j] = zo;
    }
    pbeta = beta; peps = eps; pinv2s2 = inv2s2; pcst = cst;
  }
  // w -= log q(z_0)                                      mcdboundingmachine.py:157
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float dz = z[j] - qmean[j];
    w -= -(dz * dz) / (2.0f * qstd[j] * qstd[j]) - logf(qstd[j]) - kHalfLog2Pi;
  }
  if (bad || w != w) w = INFINITY;   // weight exp(-w) = 0, like a diverged particle's loss of the forward call

  if (valid && g == 0) {
    a.out_loss[p] = w;
#pragma unroll
    for (int j = 0; j < D; ++j) a.out_z[p * D + j] = z[j];
  }

  // ---- per-wave statistics of l := w over lanes 0..15 (g == 0), fixed butterfly order -> deterministic
  const bool use = valid && g == 0;
  double cnt = (use && isfinite(w)) ? 1.0 : 0.0;
  double sm = use ? (double)w : 0.0;
  double sq = use ? (double)w * (double)w : 0.0;
  double mx = use ? -(double)w : -INFINITY;
  tile_stats_butterfly(cnt, sm, sq, mx);
  double ex = (use && mx > -INFINITY && mx < INFINITY) ? exp(-(double)w - mx) : 0.0;
  tile_stats_butterfly(ex);
  if (lane == 0) {
    double* o = a.partials + wave * CMCD_NSTATS;
    o[0] = cnt; o[1] = sm; o[2] = sq; o[3] = mx; o[4] = ex;
  }
}

// ------------------------------------------------------------------------------------------
// launcher (cmcd_host.h)
// ------------------------------------------------------------------------------------------
struct ReverseFamily {
  typedef void (*fn)(ReverseArgs);
  template <int TARGET, int ARCH, int D, int T>
  static fn get() { return reverse_traj_kernel<TARGET, ARCH, D, T>; }
};

bool reverse_available(const cmcd_desc& d, int T) { return tile_pick<ReverseFamily>(d, T) != nullptr; }

int reverse_launch(const cmcd_desc& d, const WsLayout& w, const TrajArgs& ta, const float* x, hipStream_t stream) {
  ReverseFamily::fn fn = tile_pick<ReverseFamily>(d, w.T);
  if (!fn) return fail(CMCD_ERR_UNSUPPORTED, "no reverse-chain kernel instance for this (mode, target, dim, arch, width=%s%lld)", "", w.HP);
  return tile_launch(fn, d, w, ReverseArgs{ta, x}, stream);
}

}  // namespace cmcd
