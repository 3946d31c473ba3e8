// Resumable segments of the overdamped forward chain on gfx950: bridges [k0, k1) from a caller-supplied particle state, so that
// the weights can be examined (and the particles resampled) between bridges — sequential Monte Carlo over the annealing path.
//
// The reference has no such call (it runs its chain from q to bridge K in one piece); the arithmetic is the forward call's, cut
// at a bridge.  Per particle, with the schedules beta_i, eps_i, the clip rule, the network s(., i) and q of cmcd_bound_forward
// (the same prep tables):
//
//   k0 == 0:  key chain and z_0 exactly as the forward call;  wpath = -log q(z_0);  gen = gen_0
//   k0  > 0:  z = z_in, wpath = wpath_in, gen = key_in              (the forward chain's gen_k0)
//   for i = k0 .. k1-1:  the forward call's step i:  z' ~ F_i(. | z) with the deviate of gen_i;
//                        wpath += log B_i(z | z') - log F_i(z' | z);  z <- z';  gen <- gen_{i+1}
//   lg = log gamma_k1(z):  gamma_K = p;  0 < k < K: log gamma_k = beta_{k-1} log p + (1 - beta_{k-1}) log q
//                          (log p = -inf — the many_gmm floor — gives lg = -inf whatever beta is, never 0 * inf)
//   out: z, wpath, lg, key = gen_k1;  statistics over l := -(wpath + lg)
//
// wpath is carried WITHOUT the gamma term, so segments compose without a cancellation: [0, k) then [k, K) returns the bits of
// [0, K) in z, wpath, lg and the key.  That follows from the structure, not from luck: ONE runtime-bounded rotated loop,
// m = k0 .. k1, with a single evaluation site for (grad log p, grad log q, s(z_m, .)).  The evaluation at m closes step m - 1
// when m > k0 and opens step m when m < k1; at a cut both segments run the same machine code on the same z_k (the segment
// that ends there closes step k - 1 and forms lg, the one that starts there opens step k): one extra evaluation per cut.
//
// Mapping = the wave-per-tile trajectory kernel's (cmcd_kernels.hip: traj_kernel; the network, the key-chain step, the statistics
// butterflies, the instance table and the launch are shared with cmcd_reverse.hip: cmcd_tile.h): one wave owns 16 particles
// for the whole segment, lane (g, c) holds particle c and the hidden units {16 t + 4 g + r}; layer 2 on v_mfma_f32_16x16x4_f32
// with the packed W2 A fragments streamed from LDS, layers 1 and 3 on the VALU; state, key and wpath stay in registers; one
// statistics record per tile for finalize_kernel.  A NaN stays a NaN (the divergence signal, as in the forward call).
#include "cmcd_tile.h"

namespace cmcd {

struct SegmentArgs {
  TrajArgs t;        // seeds (read when k0 == 0), params, ws, partials, lay, w, n, K, var_mode, grad_clipping, ula; the rest unused
  int32_t k0, k1;    // bridges [k0, k1), 0 <= k0 < k1 <= K
  float* z;          // [n][D]  in (k0 > 0) and out
  float* wpath;      // [n]     in (k0 > 0) and out
  uint32_t* key;     // [n][2]  in (k0 > 0) and out: gen_k0 -> gen_k1
  float* lg;         // [n]     out
};

template <int TARGET, int ARCH, int D, int T>
__global__ __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4) void segment_traj_kernel(SegmentArgs sa) {
  const TrajArgs& a = sa.t;
  constexpr int HP = 16 * T;
  constexpr int Hh = (D + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lds_w2 = lds;                    // HP*HP
  float* lds_w1z = lds_w2 + HP * HP;      // D*HP
  float* lds_w3t = lds_w1z + D * HP;      // D*HP
  float* lds_b2 = lds_w3t + D * HP;       // HP
  float* lds_b3 = lds_b2 + HP;            // 16
  float* lds_tgt = lds_b3 + 16;           // tgt_floats
  const int ks = sa.k0, ke = sa.k1, K = a.K;
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

  const int gb = g & 1;
  uint32_t k0, k1;
  float z[D];
  float w;
  if (ks == 0) {
    // ---- the forward call's start: split(PRNGKey(seed)) -> (A, B); z_0 = mean + std normal(A); gen_0 = second(split(first(split(B))))
    const int32_t seed = a.seeds[pl];
    uint32_t x0, x1;
    tile_split(0u, (uint32_t)seed, gb, x0, x1);
    uint32_t a0, a1, b0, b1;
    rows01(x0, a0, a1);
    rows01(x1, b0, b1);
    float nz[2 * Hh];
#pragma unroll
    for (int j0 = 0; j0 < Hh; j0 += 4) {
      const int j = j0 + g;  // block j encrypts (ctr[j], ctr[Hh + j]); pad counters are 0
      uint32_t y0 = j, y1 = (Hh + j < D) ? Hh + j : 0;
      threefry2x32(a0, a1, y0, y1);
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
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = qstd[j] * nz[j] + qmean[j];
    tile_split(b0, b1, gb, x0, x1);
    uint32_t c0, c1;
    rows01(x0, c0, c1);
    tile_split(c0, c1, gb, x0, x1);
    rows01(x1, k0, k1);
    // wpath = -log q(z_0)
    w = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float dz = z[j] - qmean[j];
      w -= -(dz * dz) / (2.0f * qstd[j] * qstd[j]) - logf(qstd[j]) - kHalfLog2Pi;
    }
  } else {
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = sa.z[pl * D + j];
    w = sa.wpath[pl];
    k0 = sa.key[pl * 2];
    k1 = sa.key[pl * 2 + 1];
  }

  const float clipv = a.var_mode ? 1e2f : 1e3f;
  const bool clip_p = a.grad_clipping != 0;
  const bool clip_q = clip_p && a.var_mode;
  const float fsn = a.ula ? 0.f : 1.f;           // the ULA forward kernel has no network term
  const float* bias1 = a.ws + a.w.bias1;
  const float* utab = a.ws + a.w.utab;

  // Rotated loop over the states z_k0 .. z_k1: iteration m evaluates grad log p, grad log q and the network ONCE at z_m.
  float zp[D];           // z_{m-1}
  float fk_lp = 0.f;     // log F_{m-1}(z_m | z_{m-1})
  float pbeta = 0.f, peps = 0.f, pinv2s2 = 0.f, pcst = 0.f;   // schedule row m - 1 (set when step m - 1 was opened)
  float logp = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) zp[j] = 0.f;

  for (int m = ks; m <= ke; ++m) {
    float gp[D], sn[D];
    Target<TARGET, D>::eval(z, g, lds_tgt, logp, gp);
    if (a.ula == 1) {
#pragma unroll
      for (int j = 0; j < D; ++j) sn[j] = 0.f;
    } else {
      // CAIS: s(z_m, m) serves both kernels; MCD_ULA_sn: s(z_m, m - 1) serves the backward kernel of step m - 1 only
      const int64_t row = (a.ula == 2) ? (m > 0 ? m - 1 : 0) : m;
      tile_eval_net<ARCH, D, T, tile_pf(ARCH, D, T), false>(z, bias1 + row * HP, utab + row * HP, lds_w2, lds_w1z, lds_b2,
                                                       lds_w3t, lds_b3, lane, sn);
    }
    float gq[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      gq[j] = -(z[j] - qmean[j]) * qiv[j];
      if (clip_p) gp[j] = fminf(fmaxf(gp[j], -clipv), clipv);
      if (clip_q) gq[j] = fminf(fmaxf(gq[j], -clipv), clipv);
    }

    if (m > ks) {
      // ---- backward kernel of step m - 1 at z_m: closes the step
      float bk_lp = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float ub = -1.0f * (pbeta * gp[j] + (1.0f - pbeta) * gq[j]);
        const float bk = z[j] - peps * ub + peps * sn[j];
        const float db = zp[j] - bk;
        bk_lp += -(db * db) * pinv2s2 - pcst;
      }
      w += bk_lp - fk_lp;
    }
    if (m == ke) break;

    // ---- forward kernel of step m: opens the step
    const float* scr = a.ws + a.w.sched + 8 * (int64_t)m;   // {beta, eps, sigma, log sigma + log sqrt(2 pi), 1 / (2 sigma^2), ..}
    const float beta = scr[0], eps = scr[1], sig = scr[2], cst = scr[3], inv2s2 = scr[4];
    float nz[2 * Hh];
    tile_chain_step<D>(k0, k1, g, nz);
    fk_lp = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float uf = -1.0f * (beta * gp[j] + (1.0f - beta) * gq[j]);
      const float fk = z[j] - eps * uf - eps * (fsn * sn[j]);
      const float zn = fk + sig * nz[j];
      const float df = zn - fk;
      fk_lp += -(df * df) * inv2s2 - cst;
      zp[j] = z[j];
      z[j] = zn;
    }
    pbeta = beta; peps = eps; pinv2s2 = inv2s2; pcst = cst;
  }

  // lg = log gamma_k1(z_k1): log p at the end of the chain, the geometric bridge of step k1 - 1 before it
  float lg = logp;
  if (ke < K) {
    float logq = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float dz = z[j] - qmean[j];
      logq += -(dz * dz) / (2.0f * qstd[j] * qstd[j]) - logf(qstd[j]) - kHalfLog2Pi;
    }
    const float bl = a.ws[a.w.sched + 8 * (int64_t)(ke - 1)];
    lg = (logp == -INFINITY) ? -INFINITY : bl * logp + (1.0f - bl) * logq;
  }
  const float loss = -(w + lg);

  if (valid && g == 0) {
    sa.wpath[p] = w;
    sa.lg[p] = lg;
    sa.key[p * 2] = k0;
    sa.key[p * 2 + 1] = k1;
#pragma unroll
    for (int j = 0; j < D; ++j) sa.z[p * D + j] = z[j];
  }

  // ---- per-wave statistics of l over lanes 0..15 (g == 0), fixed butterfly order -> deterministic
  const bool use = valid && g == 0;
  double cnt = (use && isfinite(loss)) ? 1.0 : 0.0;
  double sm = use ? (double)loss : 0.0;
  double sq = use ? (double)loss * (double)loss : 0.0;
  double mx = use ? -(double)loss : -INFINITY;
  tile_stats_butterfly(cnt, sm, sq, mx);
  double ex = (use && mx > -INFINITY && mx < INFINITY) ? exp(-(double)loss - mx) : 0.0;
  tile_stats_butterfly(ex);
  if (lane == 0) {
    double* o = a.partials + wave * CMCD_NSTATS;
    o[0] = cnt; o[1] = sm; o[2] = sq; o[3] = mx; o[4] = ex;
  }
}

// ------------------------------------------------------------------------------------------
// launcher (cmcd_host.h)
// ------------------------------------------------------------------------------------------
struct SegmentFamily {
  typedef void (*fn)(SegmentArgs);
  template <int TARGET, int ARCH, int D, int T>
  static fn get() { return segment_traj_kernel<TARGET, ARCH, D, T>; }
};

bool segment_available(const cmcd_desc& d, int T) { return tile_pick<SegmentFamily>(d, T) != nullptr; }

int segment_launch(const cmcd_desc& d, const WsLayout& w, const TrajArgs& ta, int32_t k0, int32_t k1, float* z, float* wpath,
                   uint32_t* key, float* lg, hipStream_t stream) {
  SegmentFamily::fn fn = tile_pick<SegmentFamily>(d, w.T);
  if (!fn) return fail(CMCD_ERR_UNSUPPORTED, "no segment kernel instance for this (mode, target, dim, arch, width=%s%lld)", "", w.HP);
  return tile_launch(fn, d, w, SegmentArgs{ta, k0, k1, z, wpath, key, lg}, stream);
}

}  // namespace cmcd
