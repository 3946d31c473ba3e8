// Batched entropic optimal transport (Sinkhorn-Knopp) between equal-size point clouds, float64 throughout: the arithmetic of
// cmcd_amd/utils.py:W2_distance (the reference's ot.sinkhorn2(a, b, M / M.max(), reg), src/utils.py:207-216), for `groups`
// independent problems in the same launches.  Parity is with the float64 restatement in tests/test_gpu_sinkhorn.py.
//
// A problem's n rows are cut into T = ceil(n / kSinkhornRows) row tiles; every launch has grid (T, groups), one workgroup
// per (tile, problem).  Launches on one stream are the only synchronisation: no grid barrier, no floating-point atomics.
//   max     per tile: max_ij ||x_i - y_j||^2, or NaN when a coordinate or weight the workgroup reads is not finite
//   build   max over the tiles; K_ij = exp(-(M_ij / max) / reg) into the workspace; u = 1/n; the tile's column partials
//           part[0][t][j] = sum_{i in tile} K_ij u_i.  A problem that cannot be solved is finished here (status 2).
//   iterate launch `it` (0-based Sinkhorn iteration), every workgroup of a problem:
//             KtU_j = sum_t part[it & 1][t][j]                               (t ascending)
//             if it - 1 was a checking iteration: err = sum_j (v_j KtU_j - b_j)^2 with v of launch it - 1; every workgroup
//               of the problem gets the same bits, so all of them stop together when err < stop_thr
//             if it == num_iter_max: the cap; stop
//             v_j = b_j / KtU_j in LDS (tile 0 also stores it, parity it & 1, for the next check and for the cost)
//             u_i = a_i / sum_j K_ij v_j for the rows of its tile          (a wave per row, lanes along the row)
//             part[(it + 1) & 1][t][j] = sum_{i in tile} K_ij u_i            (a thread per column, rows ascending)
//           so a tile of K is streamed from memory once per iteration (its second reading comes from the cache) where
//           u <- a / (K v), v <- b / (K^T u) as two products would stream all of K twice.
//   cost    per tile sum u_i K_ij v_j M_ij with M recomputed from the points, then the sum over the tiles and the record
// Every sum is taken in an order fixed by (n, kSinkhornRows, kSinkhornThreads): a problem's bits do not depend on the other
// problems of the launch, on which of them are finished, or on the stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cmcd_host.h"

namespace cmcd {

constexpr int kSkThreads = kSinkhornThreads;
constexpr int kSkWaves = kSkThreads / 64;
constexpr int kSkRows = kSinkhornRows;

// per problem, 32 bytes
struct SkState {
  int32_t done;      // 1: every workgroup of the problem returns at once
  int32_t status;    // 0 converged, 1 cap reached (or still running), 2 not solvable
  int32_t iters;     // Sinkhorn iterations carried out
  int32_t pad;
  double err;        // marginal violation at the last check (NaN before the first)
  double mx;         // max_ij ||x_i - y_j||^2
};
static_assert(sizeof(SkState) == 32, "the workspace formula of include/cmcd_hip.h counts 32 bytes per problem");

// where the pieces of the workspace start (in doubles; the formula of include/cmcd_hip.h is their sum)
struct SkLayout {
  int64_t n, T, G;
  double *K, *a, *b, *u, *v, *part, *tile;
  SkState* state;
  __host__ __device__ SkLayout(void* ws, int64_t n_, int64_t G_) : n(n_), T((n_ + kSkRows - 1) / kSkRows), G(G_) {
    double* p = static_cast<double*>(ws);
    state = reinterpret_cast<SkState*>(p); p += 4 * G;
    K = p; p += G * n * n;
    a = p; p += G * n;
    b = p; p += G * n;
    u = p; p += G * n;
    v = p; p += 2 * G * n;            // [parity][G][n]
    part = p; p += 2 * G * T * n;     // [parity][G][T][n]
    tile = p;                         // [G][T]: the tiles' maxima, later their cost sums
  }
};

int64_t sinkhorn_workspace_bytes(int64_t n, int32_t groups) {
  const int64_t G = groups, T = (n + kSkRows - 1) / kSkRows;
  const int64_t bytes = 32 * G + 8 * (G * n * n + 5 * G * n + 2 * G * T * n + G * T);
  return (bytes + 15) & ~int64_t(15);
}

__device__ __forceinline__ double sk_dist2(const double* __restrict__ xi, const double* __restrict__ yj, int dim) {
  double s = 0.0;
  for (int d = 0; d < dim; ++d) {
    const double t = xi[d] - yj[d];
    s += t * t;
  }
  return s;
}

__device__ __forceinline__ bool sk_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }   // false for NaN

// the sum of one value per thread over the workgroup, the same bits in every thread: butterfly over the wave (every level adds
// the same two numbers in both lanes), then the waves' totals in ascending order.  `red` holds kSkWaves doubles.
__device__ __forceinline__ double sk_block_sum(double x, double* red) {
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
  __syncthreads();                                  // the previous use of `red` is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < kSkWaves; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(kSkThreads) void sinkhorn_max_kernel(
    const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ a, const double* __restrict__ b,
    int32_t n, int32_t dim, void* ws, int32_t groups) {
  const SkLayout L(ws, n, groups);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.y, t = blockIdx.x;
  const int row0 = (int)t * kSkRows, rows = min(kSkRows, n - row0);
  const double* xg = x + g * n * dim;
  const double* yg = y + g * n * dim;
  __shared__ double red[kSkWaves];
  __shared__ int s_bad[kSkWaves];

  int bad = 0;
  for (int64_t e = tid; e < (int64_t)n * dim; e += kSkThreads) bad |= !sk_finite(yg[e]);
  for (int64_t e = tid; e < (int64_t)rows * dim; e += kSkThreads) bad |= !sk_finite(xg[(int64_t)row0 * dim + e]);
  if (b) for (int j = tid; j < n; j += kSkThreads) bad |= !sk_finite(b[g * n + j]);
  if (a) for (int i = tid; i < rows; i += kSkThreads) bad |= !sk_finite(a[g * n + row0 + i]);

  double mx = 0.0;
  for (int r = wave; r < rows; r += kSkWaves) {
    const double* xi = xg + (int64_t)(row0 + r) * dim;
    for (int j = lane; j < n; j += 64) mx = fmax(mx, sk_dist2(xi, yg + (int64_t)j * dim, dim));
  }
  for (int d = 32; d >= 1; d >>= 1) {
    mx = fmax(mx, __shfl_xor(mx, d));
    bad |= __shfl_xor(bad, d);
  }
  if (lane == 0) { red[wave] = mx; s_bad[wave] = bad; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kSkWaves; ++w) { mx = fmax(mx, red[w]); bad |= s_bad[w]; }
    L.tile[g * L.T + t] = bad ? (double)NAN : mx;
  }
}

__global__ __launch_bounds__(kSkThreads) void sinkhorn_build_kernel(
    const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ a, const double* __restrict__ b,
    int32_t n, int32_t dim, double reg, void* ws, int32_t groups) {
  const SkLayout L(ws, n, groups);
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.y, t = blockIdx.x, T = L.T;
  const int row0 = (int)t * kSkRows, rows = min(kSkRows, n - row0);

  double mx = 0.0;
  bool bad = false;
  for (int64_t k = 0; k < T; ++k) {
    const double m = L.tile[g * T + k];
    bad |= m != m;
    mx = fmax(mx, m);
  }
  bad |= !(mx > 0.0) || !sk_finite(mx);             // all points equal: M / max is 0 / 0; an overflowing distance
  SkState* st = L.state + g;
  if (t == 0 && tid == 0) {
    st->status = bad ? 2 : 1;
    st->iters = 0;
    st->pad = 0;
    st->err = (double)NAN;
    st->mx = bad ? (double)NAN : mx;
    __atomic_store_n(&st->done, bad ? 1 : 0, __ATOMIC_RELAXED);
  }
  if (bad) return;

  const double u0 = 1.0 / (double)n;
  const double* xg = x + g * n * dim;
  const double* yg = y + g * n * dim;
  double* Kg = L.K + g * n * n;
  for (int j = tid; j < n; j += kSkThreads) {
    const double* yj = yg + (int64_t)j * dim;
    double acc = 0.0;
    for (int r = 0; r < rows; ++r) {
      const double m = sk_dist2(xg + (int64_t)(row0 + r) * dim, yj, dim) / mx;
      const double k = exp(-m / reg);
      Kg[(int64_t)(row0 + r) * n + j] = k;
      acc += k * u0;
    }
    L.part[(g * T + t) * n + j] = acc;               // parity 0
    if (t == 0) {
      L.b[g * n + j] = b ? b[g * n + j] : u0;
      L.v[(L.G + g) * n + j] = u0;                   // parity 1 = "the v before iteration 0"
    }
  }
  for (int i = tid; i < rows; i += kSkThreads) {
    L.a[g * n + row0 + i] = a ? a[g * n + row0 + i] : u0;
    L.u[g * n + row0 + i] = u0;
  }
}

// dynamic LDS: v[n], u of the tile [kSkRows], the reduction's [kSkWaves]
__global__ __launch_bounds__(kSkThreads) void sinkhorn_iterate_kernel(int32_t n, int32_t it, int32_t num_iter_max,
                                                                      double stop_thr, void* ws, int32_t groups) {
  const SkLayout L(ws, n, groups);
  const int64_t g = blockIdx.y, t = blockIdx.x, T = L.T;
  SkState* st = L.state + g;
  if (__atomic_load_n(&st->done, __ATOMIC_RELAXED)) return;       // uniform enough: whoever reads 0 here while tile 0 sets
                                                                    // it in this launch reaches the same verdict below
  extern __shared__ double lds[];
  double* sv = lds;
  double* su = lds + n;
  double* red = su + kSkRows;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = (int)t * kSkRows, rows = min(kSkRows, n - row0);
  const int par = it & 1;
  const double* bg = L.b + g * n;
  const double* pin = L.part + ((int64_t)par * L.G + g) * T * n;
  const bool check = it >= 1 && (it - 1) % 10 == 0;
  const double* vprev = L.v + ((int64_t)(par ^ 1) * L.G + g) * n;

  // K^T u of the previous launch, tiles in ascending order; kept in LDS (as K^T u for now)
  double e = 0.0;
  for (int j = tid; j < n; j += kSkThreads) {
    double s = pin[j];
    for (int64_t k = 1; k < T; ++k) s += pin[k * n + j];
    sv[j] = s;
    if (check) {
      const double r = vprev[j] * s - bg[j];
      e += r * r;
    }
  }
  if (check) {
    const double err = sk_block_sum(e, red);
    const bool conv = err < stop_thr;
    if (t == 0 && tid == 0) {
      st->err = err;
      if (conv) { st->status = 0; __atomic_store_n(&st->done, 1, __ATOMIC_RELAXED); }
    }
    if (conv) return;
  }
  if (it >= num_iter_max) {                                         // the cap: status stays 1
    if (t == 0 && tid == 0) __atomic_store_n(&st->done, 1, __ATOMIC_RELAXED);
    return;
  }
  double* vout = L.v + ((int64_t)par * L.G + g) * n;
  for (int j = tid; j < n; j += kSkThreads) {                       // (each thread turns the entries it wrote itself)
    const double vj = bg[j] / sv[j];
    sv[j] = vj;
    if (t == 0) vout[j] = vj;
  }
  __syncthreads();

  // u_i = a_i / (K v)_i for the rows of this tile
  const double* Kt = L.K + (g * n + row0) * n;
  for (int r = wave; r < rows; r += kSkWaves) {
    const double* Kr = Kt + (int64_t)r * n;
    double s0 = 0.0, s1 = 0.0;
    int j = lane;
    for (; j + 64 < n; j += 128) {
      s0 += Kr[j] * sv[j];
      s1 += Kr[j + 64] * sv[j + 64];
    }
    if (j < n) s0 += Kr[j] * sv[j];
    double s = s0 + s1;
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) {
      const double ui = L.a[g * n + row0 + r] / s;
      su[r] = ui;
      L.u[g * n + row0 + r] = ui;
    }
  }
  __syncthreads();

  // this tile's share of K^T u for the next launch
  double* pout = L.part + (((int64_t)(par ^ 1) * L.G + g) * T + t) * n;
  for (int j = tid; j < n; j += kSkThreads) {
    double s0 = 0.0, s1 = 0.0;
    int r = 0;
    for (; r + 1 < rows; r += 2) {
      s0 += Kt[(int64_t)r * n + j] * su[r];
      s1 += Kt[(int64_t)(r + 1) * n + j] * su[r + 1];
    }
    if (r < rows) s0 += Kt[(int64_t)r * n + j] * su[r];
    pout[j] = s0 + s1;
  }
  if (t == 0 && tid == 0) st->iters = it + 1;
}

__global__ __launch_bounds__(kSkThreads) void sinkhorn_cost_tile_kernel(const double* __restrict__ x,
                                                                        const double* __restrict__ y, int32_t n, int32_t dim,
                                                                        void* ws, int32_t groups) {
  const SkLayout L(ws, n, groups);
  const int64_t g = blockIdx.y, t = blockIdx.x;
  const SkState* st = L.state + g;
  if (st->status == 2) return;
  __shared__ double red[kSkWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = (int)t * kSkRows, rows = min(kSkRows, n - row0);
  const double mx = st->mx;
  const double* xg = x + g * n * dim;
  const double* yg = y + g * n * dim;
  const double* v = L.v + ((int64_t)((st->iters - 1) & 1) * L.G + g) * n;    // the v of the last iteration carried out
  const double* Kt = L.K + (g * n + row0) * n;
  double acc = 0.0;
  for (int r = wave; r < rows; r += kSkWaves) {
    const double* xi = xg + (int64_t)(row0 + r) * dim;
    const double ui = L.u[g * n + row0 + r];
    double s = 0.0;
    for (int j = lane; j < n; j += 64)
      s += Kt[(int64_t)r * n + j] * v[j] * (sk_dist2(xi, yg + (int64_t)j * dim, dim) / mx);
    acc += ui * s;
  }
  const double tot = sk_block_sum(acc, red);
  if (tid == 0) L.tile[g * L.T + t] = tot;
}

__global__ __launch_bounds__(64) void sinkhorn_cost_final_kernel(int32_t n, void* ws, int32_t groups, double* __restrict__ out,
                                                                 int32_t* __restrict__ done_flags) {
  const SkLayout L(ws, n, groups);
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= groups) return;
  const SkState* st = L.state + g;
  double cost = (double)NAN;
  if (st->status != 2) {
    cost = 0.0;
    for (int64_t k = 0; k < L.T; ++k) cost += L.tile[g * L.T + k];
  }
  out[g * 4 + 0] = cost;
  out[g * 4 + 1] = (double)st->iters;
  out[g * 4 + 2] = st->err;
  out[g * 4 + 3] = (double)st->status;
  if (done_flags) done_flags[g] = st->done;
}

__global__ __launch_bounds__(64) void sinkhorn_flags_kernel(int32_t n, void* ws, int32_t groups, int32_t* __restrict__ done_flags) {
  const SkLayout L(ws, n, groups);
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g < groups) done_flags[g] = L.state[g].done;
}

static inline dim3 sk_grid(int64_t n, int32_t groups) {
  return dim3((uint32_t)((n + kSkRows - 1) / kSkRows), (uint32_t)groups);
}

int sinkhorn_setup_launch(const double* x, const double* y, const double* a, const double* b, int64_t n, int32_t dim,
                          int32_t groups, double reg, void* workspace, hipStream_t stream) {
  hipLaunchKernelGGL(sinkhorn_max_kernel, sk_grid(n, groups), dim3(kSkThreads), 0, stream, x, y, a, b, (int32_t)n, dim,
                     workspace, groups);
  hipLaunchKernelGGL(sinkhorn_build_kernel, sk_grid(n, groups), dim3(kSkThreads), 0, stream, x, y, a, b, (int32_t)n, dim, reg,
                     workspace, groups);
  CMCD_HIP_CHECK(hipGetLastError());
  return CMCD_OK;
}

int sinkhorn_iterate_launch(int64_t n, int32_t groups, int32_t first_iteration, int32_t count, int32_t num_iter_max,
                            double stop_thr, void* workspace, int32_t* done_flags, hipStream_t stream) {
  const size_t lds = size_t(n + kSkRows + kSkWaves) * 8;
  if (lds > 64 * 1024)
    CMCD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(sinkhorn_iterate_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // launch `num_iter_max` carries out no iteration: it takes the check that iteration num_iter_max - 1 may have left open
  // and closes the problem at the cap
  const int32_t last = first_iteration + count + (first_iteration + count == num_iter_max ? 1 : 0);
  for (int32_t it = first_iteration; it < last; ++it)
    hipLaunchKernelGGL(sinkhorn_iterate_kernel, sk_grid(n, groups), dim3(kSkThreads), lds, stream, (int32_t)n, it, num_iter_max,
                       stop_thr, workspace, groups);
  if (done_flags)
    hipLaunchKernelGGL(sinkhorn_flags_kernel, dim3((uint32_t)((groups + 63) / 64)), dim3(64), 0, stream, (int32_t)n, workspace,
                       groups, done_flags);
  CMCD_HIP_CHECK(hipGetLastError());
  return CMCD_OK;
}

int sinkhorn_cost_launch(const double* x, const double* y, int64_t n, int32_t dim, int32_t groups, void* workspace, double* out,
                         int32_t* done_flags, hipStream_t stream) {
  hipLaunchKernelGGL(sinkhorn_cost_tile_kernel, sk_grid(n, groups), dim3(kSkThreads), 0, stream, x, y, (int32_t)n, dim,
                     workspace, groups);
  hipLaunchKernelGGL(sinkhorn_cost_final_kernel, dim3((uint32_t)((groups + 63) / 64)), dim3(64), 0, stream, (int32_t)n,
                     workspace, groups, out, done_flags);
  CMCD_HIP_CHECK(hipGetLastError());
  return CMCD_OK;
}

}  // namespace cmcd
