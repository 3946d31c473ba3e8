// Importance diagnostics and systematic resampling of a weighted particle system (loss[n], z[n, dim]), w_n = exp(-loss_n):
// what every entry point of this library returns, read as particles.  No analogue in the reference (it stops at the unweighted
// z and logsumexp): parity is with the float64 restatement in tests/test_gpu_resample.py.
//
// One launch, one workgroup per group of m = n / groups consecutive rows, three passes over the group:
//   1. M = max(-loss) over the finite entries, their count, and whether any entry is NaN or -inf (the group is "diverged")
//   2. w_j = exp(-loss_j - M) in float64; inclusive cumulative sum C_j into the workspace, chunk by chunk (kResampleChunk
//      rows: scan per wave, then across the waves through LDS, plus the running sum carried from the chunks before); S2 = sum w^2
//   3. ancestors a_k = min{ j : C_j > t_k S1 }, t_k = (k + u) / m, by binary search over C; then the row copies z[a_k] -> out_z
// Every sum is taken in an order fixed by (m, the block shape): repeated calls return the same bits.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cmcd_device.h"
#include "cmcd_host.h"

namespace cmcd {

constexpr int kResampleThreads = kResampleChunk;   // one row per thread and chunk
constexpr int kResampleWaves = kResampleThreads / 64;
static_assert(kResampleThreads == 1024, "the cross-wave scan below is written for 16 waves");

// u_g = word g of jax.random.uniform(PRNGKey(seed), (groups,)): jax's original counter layout (cmcd_amd/prng.py:
// random_bits) — the counters 0..groups-1, padded to even length with 0, split in two halves that go through the
// block function side by side
__device__ __forceinline__ float resample_uniform(uint32_t seed, uint32_t g, uint32_t groups) {
  const uint32_t h = (groups + 1u) / 2u;
  const bool first = g < h;
  const uint32_t j = first ? g : g - h;
  uint32_t x0 = j, x1 = (h + j < groups) ? h + j : 0u;
  threefry2x32(0u, seed, x0, x1);
  const uint32_t bits = first ? x0 : x1;
  return __uint_as_float((bits >> 9) | 0x3F800000u) - 1.0f;   // [0, 1): minval 0, maxval 1 leave it as it is
}

template <bool VEC4>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(
    const float* __restrict__ loss, const float* __restrict__ z, int64_t m, int32_t dim, uint32_t groups, uint32_t seed,
    double* __restrict__ cum, int32_t* __restrict__ anc, float* __restrict__ out_z, double* __restrict__ out_stats) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t g = blockIdx.x;
  const int64_t row0 = (int64_t)g * m;
  const float* l = loss + row0;
  double* C = cum + row0;
  int32_t* A = anc + row0;

  __shared__ float s_max[kResampleWaves];
  __shared__ int32_t s_cnt[kResampleWaves], s_bad[kResampleWaves];
  __shared__ double s_tot[2][kResampleWaves];
  __shared__ double s_s2[kResampleWaves];
  __shared__ int32_t s_last[kResampleWaves];

  // ---- pass 1: shift, finite count, divergence
  float mx = -INFINITY;
  int32_t cnt = 0, bad = 0;
  for (int64_t j = tid; j < m; j += kResampleThreads) {
    const float v = l[j];
    if (v != v || v == -INFINITY) bad = 1;
    else if (v != INFINITY) { ++cnt; mx = fmaxf(mx, -v); }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, d));
    cnt += __shfl_xor(cnt, d);
    bad |= __shfl_xor(bad, d);
  }
  if (lane == 0) { s_max[wave] = mx; s_cnt[wave] = cnt; s_bad[wave] = bad; }
  __syncthreads();
  mx = s_max[0]; cnt = s_cnt[0]; bad = s_bad[0];
  for (int w = 1; w < kResampleWaves; ++w) { mx = fmaxf(mx, s_max[w]); cnt += s_cnt[w]; bad |= s_bad[w]; }

  double* st = out_stats + (int64_t)g * CMCD_NSTATS;
  const bool degenerate = bad || cnt == 0;      // uniform over the workgroup
  double S1 = 0.0;
  int32_t last = -1;
  if (degenerate) {
    if (tid == 0) {
      const double q = bad ? (double)NAN : 0.0;
      st[0] = q; st[1] = bad ? q : -(double)INFINITY; st[2] = q; st[3] = q; st[4] = bad ? 1.0 : 0.0;
    }
  } else {
    // ---- pass 2: weights and their cumulative sum
    const double M = (double)mx;
    double carry = 0.0, s2 = 0.0;
    int par = 0;
    for (int64_t base = 0; base < m; base += kResampleChunk, par ^= 1) {
      const int64_t j = base + tid;
      double w = 0.0;
      if (j < m) {
        w = exp(-(double)l[j] - M);               // loss = +inf: exp(-inf) = 0
        s2 += w * w;
        if (w > 0.0) last = (int32_t)j;
      }
      double inc = w;                             // inclusive scan over the wave
      for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
      }
      if (lane == 63) s_tot[par][wave] = inc;
      __syncthreads();                            // (s_tot is double-buffered by chunk parity: one barrier per chunk)
      double off = carry, tot = carry;            // every thread adds the wave totals in the same order
      for (int v = 0; v < kResampleWaves; ++v) {
        tot += s_tot[par][v];
        if (v == wave - 1) off = tot;
      }
      if (j < m) C[j] = off + inc;
      carry = tot;
    }
    S1 = carry;
    for (int d = 32; d >= 1; d >>= 1) {
      s2 += __shfl_xor(s2, d);
      last = max(last, __shfl_xor(last, d));
    }
    if (lane == 0) { s_s2[wave] = s2; s_last[wave] = last; }
    __threadfence_block();
    __syncthreads();                              // also: every C_j of the group is written
    s2 = s_s2[0]; last = s_last[0];
    for (int w = 1; w < kResampleWaves; ++w) { s2 += s_s2[w]; last = max(last, s_last[w]); }
    if (tid == 0) {
      st[0] = (double)cnt;
      st[1] = M + log(S1) - log((double)m);
      st[2] = S1 * S1 / s2;
      st[3] = 1.0 / S1;                           // the largest weight is exp(0) = 1
      st[4] = 0.0;
    }
  }
  if (!anc) return;

  // ---- pass 3: ancestors (global row numbers)
  if (degenerate) {
    for (int64_t k = tid; k < m; k += kResampleThreads) A[k] = (int32_t)(row0 + k);
  } else {
    const double u = (double)resample_uniform(seed, g, groups);
    for (int64_t k = tid; k < m; k += kResampleThreads) {
      const double thr = (((double)k + u) / (double)m) * S1;
      int64_t lo = 0, hi = last;                  // the answer is a row of positive weight: never past `last`
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (C[mid] > thr) hi = mid; else lo = mid + 1;
      }
      A[k] = (int32_t)(row0 + lo);
    }
  }
  if (!out_z) return;
  __threadfence_block();
  __syncthreads();

  // ---- row copies out_z[k, :] = z[a_k, :]
  if (dim >= 64) {                                // a wave per row, lanes along the row
    for (int64_t k = wave; k < m; k += kResampleWaves) {
      const float* src = z + (int64_t)A[k] * dim;
      float* dst = out_z + (row0 + k) * dim;
      if (VEC4) {
        for (int c = lane; c < dim / 4; c += 64)
          reinterpret_cast<float4*>(dst)[c] = reinterpret_cast<const float4*>(src)[c];
      } else {
        for (int c = lane; c < dim; c += 64) dst[c] = src[c];
      }
    }
  } else {                                        // short rows: consecutive lanes write consecutive floats
    const int64_t total = m * dim;
    for (int64_t e = tid; e < total; e += kResampleThreads) {
      const int64_t k = e / dim;
      const int c = (int)(e - k * dim);
      out_z[row0 * dim + e] = z[(int64_t)A[k] * dim + c];
    }
  }
}

static inline int64_t align16(int64_t x) { return (x + 15) & ~int64_t(15); }

// [n] float64 cumulative weights, then [n] int32 ancestors (where the row copies read them when the caller wants no index)
int64_t resample_workspace_bytes(int64_t n) { return align16(n * 8) + align16(n * 4); }

int resample_launch(const float* loss, const float* z, int64_t n, int32_t dim, int32_t groups, uint32_t seed, void* workspace,
                    int32_t* out_index, float* out_z, double* out_stats, hipStream_t stream) {
  double* cum = static_cast<double*>(workspace);
  int32_t* anc = out_index ? out_index : reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + align16(n * 8));
  if (!out_index && !out_z) anc = nullptr;        // statistics only
  const bool vec4 = out_z && dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(out_z)) & 15) == 0;
  auto kern = vec4 ? resample_kernel<true> : resample_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)groups), dim3(kResampleThreads), 0, stream, loss, z, n / groups, dim,
                     (uint32_t)groups, seed, cum, anc, out_z, out_stats);
  CMCD_HIP_CHECK(hipGetLastError());
  return CMCD_OK;
}

}  // namespace cmcd
