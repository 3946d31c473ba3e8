// UHA — Hamiltonian AIS on lgcp (d = 1600): the arithmetic of cmcd_hais.hip:1-21 (include/cmcd_hip.h, the UHA block) on the target
//   log p(z) = counts . z - a sum_j e^{z_j} - 1/2 (z - mu0)^T K^-1 (z - mu0) + lognorm,
//   grad log p(z) = -(z - mu0) K^-1 + counts - a e^z,   Hessian = -K^-1 - diag(a e^z)        (cmcd_amd/lgcp.py: lgcp_constants)
// as a launch sequence: one launch per target evaluation m = 0 .. K L, forward and backward.  The only thing an evaluation needs
// from other columns is one product of the batch with the symmetric prior precision; everything else of a leap-frog step (kicks,
// drift, momentum refresh, weight terms, every entry of d mean, d logdiag and d md) depends on the element's own column and runs in
// the product's epilogue.
//
// Product (hl_load + hl_mma): workgroup (ct, rb) owns the 16 columns [16 ct, 16 ct + 16) of the 32 particles [32 rb, 32 rb + 32),
// on v_mfma_f32_16x16x4_f32.  K^-1 is symmetric, so lane (g, c) fetches its B operand as the four consecutive k of ROW 16 ct + c
// in one 16-byte load and gives the A operand (four consecutive k of its particle's row) the same k order: no packed copy of the
// matrix.  One B fragment serves both 16-row halves; the second half is skipped when the block has at most 16 rows.  The
// contraction is split over the ten waves of the workgroup (160 k each, two accumulators per half; all of a wave's loads are issued
// before its first matrix instruction) and summed through LDS in wave order.  Afterwards waves 0 .. 7 run the epilogue, one element
// per thread: wave w, lane -> (row 32 rb + 16 (w / 4) + 4 (lane >> 4) + w % 4, column 16 ct + (lane & 15)).  A call of at most 32
// particles would leave 156 of 256 CUs idle: its two halves then go to workgroups of their own (grid.y = 2 rb + half; same
// accumulation order, so a particle's bits do not depend on which form ran).
//
// Forward (cmcd_hais_lgcp_bound_grad):
//   hl_init_kernel    z_0 = mean + sd normal(A) and w = -log q(z_0) per element, rho_prev = s normal(R); the head of every particle's
//                     key chain and its first refresh key G_0 (the keys live in [n][K][2] words; G_{i+1} is drawn by extra
//                     workgroups of the launch that opens bridge i: hl_key_step); the betas (hais_form_betas' arithmetic)
//   hl_eval_kernel    m = 0 .. K L: kr = (z - mu0) K^-1, then per element: the closing half kick of bridge i - 1 with its weight
//                     term (l == 0, m > 0), the refresh from G_i and the opening half kick (l == 0) or the full kick, the drift
//                     into the other z buffer (the next product needs whole rows: z is double-buffered).  At m = K L: log p(z_K)
//                     from the same kr and the sums of w over the tile's 16 columns into slots [n][100]
//   hl_final_kernel   the 100 slots of a particle in a fixed order -> loss; one statistics record per 16 particles
// The per-element running w, the momentum r and the refreshed momentum rho live in [n][D] buffers owned element by element.
//
// What a gradient call keeps, all [.][n][D] float32 in the workspace:
//   pos  [K L + 1]  the position of every evaluation          kr   [K L + 1]  its product (z - mu0) K^-1
//   rho  [K]        the refreshed momentum of every bridge    rend [K + 1]    as in cmcd_hais.hip
// i.e. 2 (K L + 1) + 2 K + 1 rows, plus 8 rows of sweep state.
//
// Reverse sweep (hl_sweep_kernel, m = K L .. 0): the adjoint of grad log p at evaluation m, agp_m = beta kappa ar (+ the closing
// kick's share at a boundary), is column-local in what evaluation m + 1 leaves, so the epilogue of launch m + 1 (the forward's
// last launch for m = K L) writes it as whole rows and launch m takes the ONE product pr = agp_m K^-1 (no mu0 shift):
// az += -pr - a e^z agp_m.  The rest is hais_grad_kernel's, per element.  d mean / d logdiag / d md accumulate in [n][D] buffers
// owned element by element; d eps, d eta and the two d beta shares of a launch are summed over the workgroup in a fixed order and
// stored to the slot (m, rb, ct).  hl_reduce1_kernel sums the slots of each m and the columns over the particles, hl_reduce2_kernel
// (one workgroup) writes the gradient and carries d beta through the interpolation and the normalised cumulative sum
// (hais_reduce_kernel's chain rule).  Plain stores only, no floating-point atomics, every launch on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cmcd_tile.h"

namespace cmcd {

constexpr int kHlD = 1600;              // the one width
constexpr int kHlHalf = kHlD / 2;       // normal(key, (D,)): block j encrypts (j, D / 2 + j)
constexpr int kHlTiles = kHlD / 16;     // column tiles
constexpr int kHlRows = 32;             // particles per row block
constexpr int kHlWaves = 10;            // waves of a product workgroup: the contraction is split over them ...
constexpr int kHlChunks = kHlD / 16 / kHlWaves;   // ... in chunks of 16 k, 10 per wave; waves 0 .. 3 then run the epilogue
constexpr int kHlMaxBridges = 4096;
constexpr int kHlMaxGrid = 1024;
constexpr int64_t kHlMaxN = (int64_t)1 << 20;   // gridDim.y = ceil(n / 32)

struct HlArgs {
  const int32_t* seeds;
  const float* params;
  const float* tc;            // {Kinv[D][D], counts[D], mu0, a, lognorm}
  float* out_loss;
  float* out_z;
  double* partials;           // [ceil(n / 16)][5]
  float* betas;               // [K]
  uint32_t* keys;             // [n][K][2]: the refresh key G_i of every particle
  uint32_t* gen;              // [n][2]: the key the chain goes on from (hl_key_step)
  float* wslot;               // [n][100]
  float* zbuf[2];             // [n][D] each
  float* r;                   // momentum
  float* rho;                 // refreshed momentum of the current bridge
  float* wacc;                // running w per element
  float* pos;                 // kept rows (null: forward only)
  float* kr;
  float* krho;
  float* krend;
  float* agp[2];              // sweep
  float* zb;
  float* rb;
  float* rcur;
  float* gmu;
  float* glam;
  float* gmd;
  float* scal;                // [K L + 1][row blocks][100][4]
  float* scal2;               // [K L + 1][4]
  float* colsum;              // [3][D]
  cmcd_hais_layout lay;
  int64_t n;
  int32_t K, L;
  float omega;
};

// split(key) -> (first, second)                                                     cmcd_tile.h: tile_split + rows01
__device__ __forceinline__ void hl_split(uint32_t k0, uint32_t k1, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) {
  uint32_t x0 = 0u, x1 = 2u, y0 = 1u, y1 = 3u;
  threefry2x32(k0, k1, x0, x1);
  threefry2x32(k0, k1, y0, y1);
  a0 = x0; a1 = y0; b0 = x1; b1 = y1;
}

// entry `col` of normal(key, (D,))                                                  cmcd_tile.h: tile_normal
__device__ __forceinline__ float hl_normal_at(uint32_t k0, uint32_t k1, int col) {
  const int j = col < kHlHalf ? col : col - kHlHalf;
  uint32_t y0 = (uint32_t)j, y1 = (uint32_t)(kHlHalf + j);
  threefry2x32(k0, k1, y0, y1);
  return bits_to_normal(col < kHlHalf ? y0 : y1);
}

__device__ __forceinline__ int hl_cell(const float* gx, int G, float x) {
  int j = 1;
  while (j < G + 1 && gx[j] <= x) ++j;
  return j;
}

// one step of particle p's key chain: (G, H) = split(gen); keys[p][i] = G; gen = second(split(H)).  The chain is serial (two
// dependent Threefry stages per bridge: 69 us for K = 128 when one launch walked it), so step i + 1 rides in extra workgroups of the
// evaluation launch that opens bridge i, next to the product, and costs the call nothing.
__device__ __forceinline__ void hl_key_step(const HlArgs& a, int64_t p, int i) {
  uint32_t g0, g1, h0, h1, t0, t1, k0, k1;
  hl_split(a.gen[2 * p], a.gen[2 * p + 1], g0, g1, h0, h1);
  a.keys[(p * a.K + i) * 2] = g0;
  a.keys[(p * a.K + i) * 2 + 1] = g1;
  hl_split(h0, h1, t0, t1, k0, k1);
  a.gen[2 * p] = k0;
  a.gen[2 * p + 1] = k1;
}

// ------------------------------------------------------------------------------------------
// init: blocks [0, 4 n): the element draws of particle b / 4, column pairs (j, 800 + j), j = 256 (b % 4) + thread;
// the next ceil(n / 256) blocks: the head of the key chain and G_0 of one particle per thread; the last block: the betas
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hl_init_kernel(HlArgs a) {
  __shared__ float gy[kHlMaxGrid + 2];
  const int64_t b = blockIdx.x;
  const int64_t nelem = 4 * a.n, nkey = (a.n + 255) / 256;
  if (b < nelem) {
    const int64_t p = b >> 2;
    const int j = (int)(b & 3) * 256 + (int)threadIdx.x;
    if (j >= kHlHalf) return;
    uint32_t a0, a1, b0, b1, c0, c1, t0, t1, r0, r1;
    hl_split(0u, (uint32_t)a.seeds[p], a0, a1, b0, b1);   // (A, B) = split(PRNGKey(seed))
    hl_split(b0, b1, c0, c1, t0, t1);                     // C = first(split(B))
    hl_split(c0, c1, r0, r1, t0, t1);                     // (R, G') = split(C)
    uint32_t e0 = (uint32_t)j, e1 = (uint32_t)(kHlHalf + j), m0 = e0, m1 = e1;
    threefry2x32(a0, a1, e0, e1);
    threefry2x32(r0, r1, m0, m1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int col = j + h * kHlHalf;
      const int64_t idx = p * kHlD + col;
      const float mean = a.params[a.lay.vd_mean + col], ld = a.params[a.lay.vd_logdiag + col];
      const float sd = expf(ld), sm = expf(a.params[a.lay.md + col]);
      const float z = sd * bits_to_normal(h ? e1 : e0) + mean;
      const float dz = z - mean;
      a.zbuf[0][idx] = z;
      a.wacc[idx] = -(-(dz * dz) / (2.0f * sd * sd) - ld - kHalfLog2Pi);   // w = -log q(z_0), this column's term
      const float r = sm * bits_to_normal(h ? m1 : m0);                     // rho_prev = s normal(R)
      a.r[idx] = r;
      if (a.pos) a.krend[idx] = r;
    }
  } else if (b < nelem + nkey) {
    const int64_t p = (b - nelem) * 256 + threadIdx.x;
    if (p >= a.n) return;
    uint32_t a0, a1, b0, b1, c0, c1, t0, t1, r0, r1, p0, p1, k0, k1;
    hl_split(0u, (uint32_t)a.seeds[p], a0, a1, b0, b1);
    hl_split(b0, b1, c0, c1, t0, t1);
    hl_split(c0, c1, r0, r1, p0, p1);
    hl_split(p0, p1, t0, t1, k0, k1);                     // gen = second(split(G'))
    a.gen[2 * p] = k0;
    a.gen[2 * p + 1] = k1;
    hl_key_step(a, p, 0);                                 // G_0; every later G_i comes from the launch that opens bridge i - 1
  } else {
    // betas[K] = interp(target_x, gridref_x, [0, cumsum(mgridref_y) / sum]): cmcd_hais.hip's hais_form_betas
    const int G = (int)a.lay.ngrid;
    const float* ms = a.params + a.lay.mgridref_y;
    const float* gx = a.params + a.lay.gridref_x;
    if (threadIdx.x == 0) {
      float run = 0.f;
      gy[0] = 0.f;
      for (int q = 0; q <= G; ++q) {
        run += ms[q];
        gy[q + 1] = run;
      }
      for (int q = 1; q <= G + 1; ++q) gy[q] = gy[q] / run;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.K; i += blockDim.x) {
      const float x = a.params[a.lay.target_x + i];
      const int j = hl_cell(gx, G, x);
      a.betas[i] = gy[j - 1] + ((x - gx[j - 1]) / (gx[j] - gx[j - 1])) * (gy[j] - gy[j - 1]);
    }
  }
}

// ------------------------------------------------------------------------------------------
// the product of the row block with K^-1 (see the head of the file), in two steps so that a kernel can put work between the
// loads and the matrix instructions.  `split`: blockIdx.y = 2 rb + h and the workgroup takes the 16-row half h alone.
// ------------------------------------------------------------------------------------------
struct HlTile {
  int64_t base;        // first particle of the row block
  int cbase;           // first column of the tile
  bool do0, do1;       // which halves this workgroup computes (uniform)
  // the element this thread owns in the epilogue (waves 0 .. 7: wave w takes half w / 4, accumulator register w % 4)
  int eh, eq, col;
  int64_t p;
  bool active;
};
__device__ __forceinline__ HlTile hl_tile(int64_t n, int split) {
  HlTile t;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t rb = split ? blockIdx.y >> 1 : blockIdx.y;
  t.base = rb * kHlRows;
  t.cbase = blockIdx.x * 16;
  const bool two = n - t.base > 16;
  t.do0 = !split || (blockIdx.y & 1) == 0;
  t.do1 = two && (!split || (blockIdx.y & 1) == 1);
  t.eh = (wv >> 2) & 1;
  t.eq = wv & 3;
  t.col = t.cbase + (lane & 15);
  t.p = t.base + 16 * t.eh + 4 * (lane >> 4) + t.eq;
  t.active = wv < 8 && t.p < n && (t.eh ? t.do1 : t.do0);
  return t;
}

struct HlFrag {
  f32x4 bv[kHlChunks], av[kHlChunks], aw[kHlChunks];
};
// every load of the wave's share is issued before the first matrix instruction: one memory latency per launch, not one per chunk
__device__ __forceinline__ void hl_load(const float* __restrict__ x, const float* __restrict__ kinv, int64_t n, const HlTile& t,
                                        HlFrag& f) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t p0 = t.base + c < n ? t.base + c : n - 1, p1 = t.base + 16 + c < n ? t.base + 16 + c : n - 1;   // padding rows read row n - 1
  const float* xa = x + p0 * kHlD + wv * (16 * kHlChunks) + 4 * g;
  const float* xb = x + p1 * kHlD + wv * (16 * kHlChunks) + 4 * g;
  const float* bp = kinv + (int64_t)(t.cbase + c) * kHlD + wv * (16 * kHlChunks) + 4 * g;
#pragma unroll
  for (int ch = 0; ch < kHlChunks; ++ch) {
    f.bv[ch] = *reinterpret_cast<const f32x4*>(bp + 16 * ch);
    f.av[ch] = t.do0 ? *reinterpret_cast<const f32x4*>(xa + 16 * ch) : f32x4{0.f, 0.f, 0.f, 0.f};
    f.aw[ch] = t.do1 ? *reinterpret_cast<const f32x4*>(xb + 16 * ch) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}
// -> this thread's element (t.eh, t.eq, lane) of X K^-1, the waves' shares added in wave order.  Ends behind a barrier.
template <bool SHIFT>
__device__ __forceinline__ float hl_mma(HlFrag& f, float shift, const HlTile& t, float* lds) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  f32x4 acc[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[h][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ch = 0; ch < kHlChunks; ++ch) {
    if (t.do0) {
      if (SHIFT) f.av[ch] -= shift;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[0][q & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.av[ch][q], f.bv[ch][q], acc[0][q & 1], 0, 0, 0);
    }
    if (t.do1) {
      if (SHIFT) f.aw[ch] -= shift;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[1][q & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.aw[ch][q], f.bv[ch][q], acc[1][q & 1], 0, 0, 0);
    }
  }
  // lds[wave][half][reg][lane]
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x4 s = acc[h][0] + acc[h][1];
#pragma unroll
    for (int q = 0; q < 4; ++q) lds[((wv * 2 + h) * 4 + q) * 64 + lane] = s[q];
  }
  __syncthreads();
  float s = 0.f;
  if (wv < 8) {
    s = lds[((0 * 2 + t.eh) * 4 + t.eq) * 64 + lane];
#pragma unroll
    for (int w = 1; w < kHlWaves; ++w) s += lds[((w * 2 + t.eh) * 4 + t.eq) * 64 + lane];
  }
  return s;
}

// the per-column constants of q and of the momentum distribution
struct HlCol {
  float mean, qiv, sm, iv, cnt;
};
__device__ __forceinline__ HlCol hl_col(const HlArgs& a, int col) {
  HlCol k;
  k.mean = a.params[a.lay.vd_mean + col];
  const float sd = expf(a.params[a.lay.vd_logdiag + col]);
  k.qiv = 1.0f / (sd * sd);
  k.sm = expf(a.params[a.lay.md + col]);
  k.iv = 1.0f / (k.sm * k.sm);
  k.cnt = a.tc[(int64_t)kHlD * kHlD + col];
  return k;
}

// ------------------------------------------------------------------------------------------
// forward: evaluation m = i L + l (m == K L: i = K, l = 0).  What the epilogue reads is requested first, the product's operands
// second, and the refresh deviate is drawn while they are on their way.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kHlWaves) void hl_eval_kernel(HlArgs a, int m, int i, int l, int split) {
  __shared__ __attribute__((aligned(16))) float lds[kHlWaves * 2 * 4 * 64];
  if (blockIdx.x >= kHlTiles) {   // the extra workgroups of a launch that opens bridge i < K - 1: the key of bridge i + 1
    const int64_t p = (int64_t)(blockIdx.x - kHlTiles) * (64 * kHlWaves) + threadIdx.x;
    if (blockIdx.y == 0 && p < a.n) hl_key_step(a, p, i + 1);
    return;
  }
  const int lane = threadIdx.x & 63;
  const HlTile t = hl_tile(a.n, split);
  const int ct = blockIdx.x, col = t.col;
  const int64_t nD = a.n * kHlD;
  const float mu0 = a.tc[(int64_t)kHlD * kHlD + kHlD], aa = a.tc[(int64_t)kHlD * kHlD + kHlD + 1];
  const float* zin = a.zbuf[m & 1];
  float* zout = a.zbuf[(m + 1) & 1];
  const int M = a.K * a.L;
  const bool closing = m > 0 && l == 0, last = m == M, keep = a.pos != nullptr;
  const bool refresh = !last && l == 0;
  const int64_t idx = t.p * kHlD + col;
  float z = 0.f, r = 0.f, w = 0.f, rho_c = 0.f;
  uint32_t key0 = 0u, key1 = 0u;
  if (t.active) {
    z = zin[idx];
    r = a.r[idx];
    w = a.wacc[idx];
    if (closing) rho_c = a.rho[idx];
    if (refresh) {
      const uint32_t* key = a.keys + (t.p * a.K + i) * 2;
      key0 = key[0];
      key1 = key[1];
    }
  }
  const HlCol k = hl_col(a, col);
  const float eps = a.params[a.lay.eps], eta = a.params[a.lay.eta];
  const float bp = closing ? a.betas[i - 1] : 0.f, be = last ? 0.f : a.betas[i];
  HlFrag f;
  hl_load(zin, a.tc, a.n, t, f);
  float xi = 0.f;
  if (t.active && refresh) xi = hl_normal_at(key0, key1, col);
  const float kr = hl_mma<true>(f, mu0, t, lds);
  const float ce = sqrtf(1.0f - eta * eta);
  if (t.active) {
    const float ez = aa * expf(z);
    const float gp = -kr + k.cnt - ez;
    const float gq = -(z - k.mean) * k.qiv;
    if (keep) {
      a.pos[(int64_t)m * nD + idx] = z;
      a.kr[(int64_t)m * nD + idx] = kr;
    }
    if (closing) {   // the closing half kick of bridge i - 1 and its weight
      const float gU = -1.0f * (bp * gp + (1.0f - bp) * gq);
      r -= 0.5f * eps * gU;
      w += 0.5f * ((rho_c - r) * (rho_c + r) * k.iv);
      if (keep) a.krend[(int64_t)i * nD + idx] = r;
    }
    if (last) {
      w += k.cnt * z - ez - 0.5f * ((z - mu0) * kr);   // this column's term of log p(z_K)
      a.out_z[idx] = z;
      if (keep) a.agp[m & 1][idx] = bp * 0.5f * eps * (a.omega * r * k.iv);   // the sweep's first product operand
    } else {
      const float gU = -1.0f * (be * gp + (1.0f - be) * gq);
      if (l == 0) {
        const float rho = eta * r + ce * k.sm * xi;
        r = rho - 0.5f * eps * gU;
        a.rho[idx] = rho;
        if (keep) a.krho[(int64_t)i * nD + idx] = rho;
      } else {
        r -= eps * gU;
      }
      zout[idx] = z + eps * r * k.iv;
      a.r[idx] = r;
      a.wacc[idx] = w;
    }
  }
  if (last) {   // uniform: the sum of w over the 16 columns of the tile, in a fixed order
    if (!t.active) w = 0.f;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) w += __shfl_xor(w, o);
    if (t.active && (lane & 15) == 0) a.wslot[t.p * kHlTiles + ct] = w;
  }
}

__global__ __launch_bounds__(256) void hl_final_kernel(HlArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = p < a.n;
  float loss = 0.f;
  if (valid) {
    const float* s = a.wslot + p * kHlTiles;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < kHlTiles; q += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += s[q + u];
    }
    const float w = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + a.tc[(int64_t)kHlD * kHlD + kHlD + 2];
    loss = -w;
    a.out_loss[p] = loss;
  }
  const int64_t tile = p >> 4;
  if (tile * 16 < a.n)   // uniform over the 16 lanes of a record
    tile_stats_record(loss, valid, (int)(threadIdx.x & 15), a.partials + tile * CMCD_NSTATS);
}

// ------------------------------------------------------------------------------------------
// reverse sweep: evaluation m = i L + l.  Per element hais_grad_kernel's order: drift, opening kick (at the head of a bridge the
// refresh and its weight term), closing kick of the previous bridge (and its weight term), then the Hessians.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kHlWaves) void hl_sweep_kernel(HlArgs a, int m, int i, int l, int split) {
  __shared__ __attribute__((aligned(16))) float lds[kHlWaves * 2 * 4 * 64];
  __shared__ float lds_s[4][8];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const HlTile t = hl_tile(a.n, split);
  const int ct = blockIdx.x, col = t.col;
  const int64_t nD = a.n * kHlD;
  const float aa = a.tc[(int64_t)kHlD * kHlD + kHlD + 1];
  const int K = a.K, L = a.L, M = K * L;
  const bool first = m == M, closing = m > 0 && l == 0;
  // the evaluation the next launch undoes: m - 1 = i' L + l'
  const int i1 = l > 0 ? i : i - 1, l1 = l > 0 ? l - 1 : L - 1;
  const bool closing1 = m - 1 > 0 && l1 == 0;
  const int64_t idx = t.p * kHlD + col;
  float z = 0.f, kr = 0.f, a_gp = 0.f, zb = 0.f, rb = 0.f, r = 0.f, gmu = 0.f, glam = 0.f, gmd = 0.f, re = 0.f, rh = 0.f;
  float rh1 = 0.f, re1 = 0.f;
  if (t.active) {
    z = a.pos[(int64_t)m * nD + idx];
    kr = a.kr[(int64_t)m * nD + idx];
    a_gp = a.agp[m & 1][idx];   // what the product takes
    if (!first) {
      zb = a.zb[idx]; rb = a.rb[idx]; r = a.rcur[idx];
      gmu = a.gmu[idx]; glam = a.glam[idx]; gmd = a.gmd[idx];
    }
    if (l == 0) re = a.krend[(int64_t)i * nD + idx];   // what enters bridge i = what left bridge i - 1
    if (!first && l == 0) rh = a.krho[(int64_t)i * nD + idx];
    if (closing1) {
      rh1 = a.krho[(int64_t)i1 * nD + idx];
      re1 = a.krend[(int64_t)i1 * nD + idx];
    }
  }
  const HlCol k = hl_col(a, col);
  const float eps = a.params[a.lay.eps], eta = a.params[a.lay.eta], om = a.omega;
  const float be = first ? 0.f : a.betas[i], bp = closing ? a.betas[i - 1] : 0.f;
  const float be1 = m > 0 ? a.betas[i1] : 0.f, bp1 = closing1 ? a.betas[i1 - 1] : 0.f;
  HlFrag f;
  hl_load(a.agp[m & 1], a.tc, a.n, t, f);
  const float pr = hl_mma<false>(f, 0.f, t, lds);
  const float ic2 = 1.0f / (1.0f - eta * eta);
  const float kap = l == 0 ? 0.5f * eps : eps, kf = l == 0 ? 0.5f : 1.0f;
  const float kap1 = l1 == 0 ? 0.5f * eps : eps;
  float s_eps = 0.f, s_eta = 0.f, s_open = 0.f, s_close = 0.f;
  if (t.active) {
    const float ez = aa * expf(z);
    const float gp = -kr + k.cnt - ez;
    const float gq = -(z - k.mean) * k.qiv;
    float a_gq = 0.f, geps = 0.f, geta = 0.f;
    if (!first) {
      const float gU = -1.0f * (be * gp + (1.0f - be) * gq);
      // drift z' = z + eps r / s^2 with r = the momentum after this evaluation's kick
      const float tt = zb * r * k.iv;
      rb += eps * k.iv * zb;
      geps += tt;
      gmd -= 2.0f * eps * tt;
      // kick r = r_in - kap gU
      a_gq += (1.0f - be) * kap * rb;
      s_open += kap * ((gp - gq) * rb);
      geps -= kf * gU * rb;
      r += kap * gU;          // the momentum before the kick
      if (l == 0) {
        // refresh rho = eta rho_prev + sqrt(1 - eta^2) s xi and the weight term -rho^2 / (2 s^2) of the loss
        const float rhob = rb - om * rh * k.iv;
        gmd += om * rh * rh * k.iv;
        const float dv = rh - eta * re;          // sqrt(1 - eta^2) s xi
        geta += rhob * (re - eta * ic2 * dv);
        gmd += rhob * dv;
        rb = eta * rhob;
        if (m == 0) gmd += rb * re;              // rend[0] = s normal(R)
      }
    }
    if (closing) {   // closing half kick of bridge i - 1: r_end = r - eps/2 gU, loss += r_end^2 / (2 s^2)
      const float gU = -1.0f * (bp * gp + (1.0f - bp) * gq);
      rb += om * re * k.iv;
      gmd -= om * re * re * k.iv;
      a_gq += (1.0f - bp) * 0.5f * eps * rb;
      s_close += 0.5f * eps * ((gp - gq) * rb);
      geps -= 0.5f * gU * rb;
      r = re + 0.5f * eps * gU;
    }
    if (first) zb -= om * gp;                    // loss -= log p(z_K)
    zb += (-pr - ez * a_gp) - a_gq * k.qiv;
    gmu += a_gq * k.qiv;
    glam += a_gq * (-2.0f * gq);
    if (m == 0) {   // z_0 = mean + std e,  log q(z_0) = -|e|^2 / 2 - sum logdiag - const
      gmu += zb;
      glam += zb * (z - k.mean) - om;
    }
    a.gmu[idx] = gmu; a.glam[idx] = glam; a.gmd[idx] = gmd;
    s_eps = geps;
    s_eta = geta;
    if (m > 0) {
      a.zb[idx] = zb; a.rb[idx] = rb; a.rcur[idx] = r;
      // the adjoint of grad log p at evaluation m - 1: the same steps on this element, up to the kicks' shares
      float rb1 = rb + eps * k.iv * zb;
      float g1 = be1 * kap1 * rb1;
      if (closing1) {
        const float rhob = rb1 - om * rh1 * k.iv;
        rb1 = eta * rhob;
        rb1 += om * re1 * k.iv;
        g1 += bp1 * 0.5f * eps * rb1;
      }
      a.agp[(m - 1) & 1][idx] = g1;
    }
  }
  // the four scalars of this launch over the workgroup's elements: lanes, then the eight epilogue waves, in a fixed order
  float v[4] = {s_eps, s_eta, s_open, s_close};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v[q] += __shfl_xor(v[q], o);
    if (lane == 0 && wv < 8) lds_s[q][wv] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int q = threadIdx.x;
    const int64_t slot = ((int64_t)m * gridDim.y + blockIdx.y) * kHlTiles + ct;
    a.scal[slot * 4 + q] = ((lds_s[q][0] + lds_s[q][1]) + (lds_s[q][2] + lds_s[q][3])) +
                           ((lds_s[q][4] + lds_s[q][5]) + (lds_s[q][6] + lds_s[q][7]));
  }
}

// blocks [0, K L]: the slots of launch m -> scal2[m][4]; the next ceil(D / 256) blocks: d mean / d logdiag / d md over the particles
__global__ __launch_bounds__(256) void hl_reduce1_kernel(HlArgs a, int64_t slots_per_m) {
  __shared__ float red[256][4];
  const int M = a.K * a.L;
  if ((int)blockIdx.x <= M) {
    const float* s = a.scal + (int64_t)blockIdx.x * slots_per_m * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t o = threadIdx.x; o < slots_per_m; o += 256) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += s[o * 4 + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[threadIdx.x][q] = acc[q];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
      if ((int)threadIdx.x < w) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[threadIdx.x][q] += red[threadIdx.x + w][q];
      }
      __syncthreads();
    }
    if (threadIdx.x < 4) a.scal2[(int64_t)blockIdx.x * 4 + threadIdx.x] = red[0][threadIdx.x];
  } else {
    const int col = ((int)blockIdx.x - M - 1) * 256 + (int)threadIdx.x;
    if (col >= kHlD) return;
    const float* src[3] = {a.gmu, a.glam, a.gmd};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};   // particle p goes to chain p % 4, the chains are added in a fixed tree
      int64_t p = 0;
      for (; p + 4 <= a.n; p += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += src[q][(p + u) * kHlD + col];
      }
      for (; p < a.n; ++p) acc[0] += src[q][p * kHlD + col];
      a.colsum[q * kHlD + col] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
  }
}

// one workgroup: zero grad, the leaves, d beta -> d mgridref_y (cmcd_hais.hip: hais_reduce_kernel)
__global__ __launch_bounds__(256) void hl_reduce2_kernel(HlArgs a, float* grad, int64_t n_params) {
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];   // gbeta[K], frac[K], cell[K], ggy[G + 2], gy[G + 2]
  __shared__ float red[256][2];
  const int K = a.K, L = a.L, M = K * L, G = (int)a.lay.ngrid;
  float* gbeta = lds_dyn;
  float* frac = lds_dyn + K;
  int* cell = reinterpret_cast<int*>(lds_dyn + 2 * K);
  float* ggy = lds_dyn + 3 * K;
  float* gy = ggy + (G + 2);
  for (int64_t o = threadIdx.x; o < n_params; o += blockDim.x) grad[o] = 0.f;
  __syncthreads();
  for (int c = threadIdx.x; c < kHlD; c += blockDim.x) {
    grad[a.lay.vd_mean + c] = a.colsum[c];
    grad[a.lay.vd_logdiag + c] = a.colsum[kHlD + c];
    grad[a.lay.md + c] = a.colsum[2 * kHlD + c];
  }
  float e0 = 0.f, e1 = 0.f;
  for (int m = threadIdx.x; m <= M; m += 256) {
    e0 += a.scal2[(int64_t)m * 4];
    e1 += a.scal2[(int64_t)m * 4 + 1];
  }
  red[threadIdx.x][0] = e0;
  red[threadIdx.x][1] = e1;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[threadIdx.x][0] += red[threadIdx.x + w][0];
      red[threadIdx.x][1] += red[threadIdx.x + w][1];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    grad[a.lay.eps] = red[0][0];
    grad[a.lay.eta] = red[0][1];
  }
  const float* gx = a.params + a.lay.gridref_x;
  const float* ms = a.params + a.lay.mgridref_y;
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    float v = 0.f;   // the kicks of bridge i in sweep order: its closing kick first
    v += a.scal2[(int64_t)(i + 1) * L * 4 + 3];
    for (int m = (i + 1) * L - 1; m >= i * L; --m) v += a.scal2[(int64_t)m * 4 + 2];
    gbeta[i] = v;
    const float x = a.params[a.lay.target_x + i];
    const int j = hl_cell(gx, G, x);
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
      grad[a.lay.mgridref_y + rr] = (suffix - dot) / S;
    }
  }
}

struct HlWs {   // offsets in floats
  int64_t partials, betas, keys, gen, wslot, z0, z1, r, rho, wacc, pos, kr, krho, krend, agp0, agp1, zb, rb, rcur, gmu, glam, gmd, scal,
      scal2, colsum, total;
};
// a call of at most one row block leaves most of the device idle: its two 16-row halves then go to workgroups of their own
static bool hl_halves_apart(int64_t n) { return n <= kHlRows; }
static int64_t hl_grid_y(int64_t n) { return hl_halves_apart(n) ? (n > 16 ? 2 : 1) : (n + kHlRows - 1) / kHlRows; }

static HlWs hl_ws(int K, int L, int64_t n, bool with_grad) {
  const int64_t tiles = (n + 15) / 16, nD = n * kHlD, M1 = (int64_t)K * L + 1, rbs = hl_grid_y(n);
  HlWs w{};
  int64_t o = 0;
  auto take = [&](int64_t len) { const int64_t at = o; o += al4(len); return at; };
  w.partials = take(tiles * CMCD_NSTATS * 2);
  w.betas = take(K);
  w.keys = take(n * K * 2);
  w.gen = take(n * 2);
  w.wslot = take(n * kHlTiles);
  w.z0 = take(nD); w.z1 = take(nD); w.r = take(nD); w.rho = take(nD); w.wacc = take(nD);
  if (with_grad) {
    w.pos = take(M1 * nD); w.kr = take(M1 * nD); w.krho = take((int64_t)K * nD); w.krend = take((int64_t)(K + 1) * nD);
    w.agp0 = take(nD); w.agp1 = take(nD); w.zb = take(nD); w.rb = take(nD); w.rcur = take(nD);
    w.gmu = take(nD); w.glam = take(nD); w.gmd = take(nD);
    w.scal = take(M1 * rbs * kHlTiles * 4);
    w.scal2 = take(M1 * 4);
    w.colsum = take(3 * kHlD);
  }
  w.total = o;
  return w;
}

static bool hl_shape_ok(int32_t nbridges, int32_t lfsteps, int64_t n) {
  return nbridges >= 1 && lfsteps >= 1 && n >= 1 && n <= kHlMaxN && nbridges <= kHlMaxBridges &&
         (int64_t)nbridges * lfsteps <= ((int64_t)1 << 24);
}

}  // namespace cmcd

using namespace cmcd;

extern "C" {

int64_t cmcd_hais_lgcp_workspace_bytes(int32_t dim, int32_t nbridges, int32_t lfsteps, int64_t n, int32_t with_grad) {
  if (nbridges < 1 || lfsteps < 1) {
    fail_msg(CMCD_ERR_BAD_ARG, "nbridges and lfsteps must be >= 1");
    return 0;
  }
  if (n < 1 || dim < 1) {
    fail_msg(CMCD_ERR_BAD_ARG, "n or dim out of range");
    return 0;
  }
  if (dim != kHlD) {
    fail_msg(CMCD_ERR_UNSUPPORTED, "no Hamiltonian AIS lgcp kernel for this dim (1600 only)");
    return 0;
  }
  if (!hl_shape_ok(nbridges, lfsteps, n)) {
    fail_msg(CMCD_ERR_UNSUPPORTED, "nbridges above 4096, nbridges * lfsteps above 2^24 or n above 2^20");
    return 0;
  }
  return hl_ws(nbridges, lfsteps, n, with_grad != 0).total * 4;
}

int cmcd_hais_lgcp_bound_grad(int32_t dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout* lay, const int32_t* seeds,
                              int64_t n, const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                              float omega, void* workspace, int64_t workspace_bytes, float* out_loss, float* out_z,
                              double* out_stats, float* grad, void* stream_) {
  if (!lay || !seeds || !params || !target_consts || !workspace || !out_loss || !out_z || !out_stats)
    return fail_msg(CMCD_ERR_BAD_ARG, "null pointer argument");
  if (nbridges < 1 || lfsteps < 1) return fail_msg(CMCD_ERR_BAD_ARG, "nbridges and lfsteps must be >= 1");
  if (n < 1 || dim < 1) return fail_msg(CMCD_ERR_BAD_ARG, "n or dim out of range");
  if (dim != kHlD) return fail_msg(CMCD_ERR_UNSUPPORTED, "no Hamiltonian AIS lgcp kernel for this dim (1600 only)");
  if (!hl_shape_ok(nbridges, lfsteps, n))
    return fail_msg(CMCD_ERR_UNSUPPORTED, "nbridges above 4096, nbridges * lfsteps above 2^24 or n above 2^20");
  if (n_target != (int64_t)dim * dim + dim + 3)
    return fail_msg(CMCD_ERR_BAD_ARG, "lgcp needs target_consts = {Kinv[dim, dim], counts[dim], mu0, a, lognorm}");
  if (reinterpret_cast<uintptr_t>(target_consts) & 15)
    return fail_msg(CMCD_ERR_BAD_ARG, "target_consts must be 16-byte aligned");
  if (lay->ngrid < 0 || lay->ngrid > kHlMaxGrid) return fail_msg(CMCD_ERR_BAD_ARG, "ngrid out of range (0 .. 1024)");
  auto inside = [&](int64_t off, int64_t len) { return off >= 0 && off + len <= n_params; };
  if (!(inside(lay->vd_mean, dim) && inside(lay->vd_logdiag, dim) && inside(lay->eps, 1) && inside(lay->eta, 1) &&
        inside(lay->md, dim) && inside(lay->mgridref_y, lay->ngrid + 1) && inside(lay->gridref_x, lay->ngrid + 2) &&
        inside(lay->target_x, nbridges)))
    return fail_msg(CMCD_ERR_BAD_ARG, "layout offset missing or outside params_flat");
  const HlWs w = hl_ws(nbridges, lfsteps, n, grad != nullptr);
  if (workspace_bytes < w.total * 4 || (reinterpret_cast<uintptr_t>(workspace) & 15))
    return fail_msg(CMCD_ERR_WORKSPACE, "workspace too small or not 16-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* ws = static_cast<float*>(workspace);
  const int64_t tiles = (n + 15) / 16, rbs = hl_grid_y(n);
  const int split = hl_halves_apart(n) ? 1 : 0;
  const int K = nbridges, L = lfsteps, M = K * L;
  HlArgs a{};
  a.seeds = seeds; a.params = params; a.tc = target_consts; a.out_loss = out_loss; a.out_z = out_z;
  a.partials = reinterpret_cast<double*>(ws + w.partials);
  a.betas = ws + w.betas; a.keys = reinterpret_cast<uint32_t*>(ws + w.keys); a.gen = reinterpret_cast<uint32_t*>(ws + w.gen); a.wslot = ws + w.wslot;
  a.zbuf[0] = ws + w.z0; a.zbuf[1] = ws + w.z1; a.r = ws + w.r; a.rho = ws + w.rho; a.wacc = ws + w.wacc;
  if (grad) {
    a.pos = ws + w.pos; a.kr = ws + w.kr; a.krho = ws + w.krho; a.krend = ws + w.krend;
    a.agp[0] = ws + w.agp0; a.agp[1] = ws + w.agp1; a.zb = ws + w.zb; a.rb = ws + w.rb; a.rcur = ws + w.rcur;
    a.gmu = ws + w.gmu; a.glam = ws + w.glam; a.gmd = ws + w.gmd;
    a.scal = ws + w.scal; a.scal2 = ws + w.scal2; a.colsum = ws + w.colsum;
  }
  a.lay = *lay; a.n = n; a.K = K; a.L = L; a.omega = omega;
  const dim3 grid((unsigned)kHlTiles, (unsigned)rbs);
  hipLaunchKernelGGL(hl_init_kernel, dim3((unsigned)(4 * n + (n + 255) / 256 + 1)), dim3(256), 0, stream, a);
  const unsigned key_blocks = (unsigned)((n + 64 * kHlWaves - 1) / (64 * kHlWaves));
  for (int m = 0; m <= M; ++m) {
    const bool opens = m % L == 0 && m / L + 1 < K;   // this launch also draws the key of the next bridge
    hipLaunchKernelGGL(hl_eval_kernel, dim3((unsigned)kHlTiles + (opens ? key_blocks : 0u), (unsigned)rbs), dim3(64 * kHlWaves), 0, stream,
                       a, m, m / L, m % L, split);
  }
  hipLaunchKernelGGL(hl_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  int rc = launch_finalize(a.partials, (int32_t)tiles, out_stats, stream_);
  if (rc != CMCD_OK) return rc;
  if (grad) {
    for (int m = M; m >= 0; --m) hipLaunchKernelGGL(hl_sweep_kernel, grid, dim3(64 * kHlWaves), 0, stream, a, m, m / L, m % L, split);
    hipLaunchKernelGGL(hl_reduce1_kernel, dim3((unsigned)(M + 1 + (kHlD + 255) / 256)), dim3(256), 0, stream, a,
                       rbs * (int64_t)kHlTiles);
    const size_t rlds = sizeof(float) * (3 * (size_t)K + 2 * ((size_t)lay->ngrid + 2));
    hipLaunchKernelGGL(hl_reduce2_kernel, dim3(1), dim3(256), rlds, stream, a, grad, n_params);
  }
  return hipGetLastError() == hipSuccess ? CMCD_OK : fail_msg(CMCD_ERR_HIP, "launch failed");
}

}  // extern "C"
