/*
 * cmcd_hip.h — C ABI of libcmcd_hip.so: the MI355X (gfx950) implementation of CMCD's
 * annealed-Langevin bound evaluation (`MCD_CAIS_sn` / `MCD_CAIS_var_sn`).
 *
 * The reference is pure Python/JAX and has no FFI; the "interface each entry point
 * replaces" is therefore the jitted Python callable the reference builds around the path:
 *
 *   cmcd_bound_forward   <->  loss_fn = jax.jit(partial(mcdbm.compute_bound[_var], eps_schedule=…,
 *                             grad_clipping=…), static_argnums=(2,3,4))
 *                             /root/reference/src/main.py:161-177, called positionally as
 *                             f(seeds, params_flat, unflatten, params_fixed, log_prob_model) at
 *                             /root/reference/src/opt.py:97-99,102-104,188-190; body
 *                             /root/reference/src/mcdboundingmachine.py:126-231 ->
 *                             /root/reference/src/mcd_utils.py:134-161 ->
 *                             /root/reference/src/mcd_cais.py:6-99 / mcd_cais_var.py:7-112.
 *   cmcd_desc            <->  params_fixed = (dim, nbridges, mode, apply_fun_sn)
 *                             (/root/reference/src/mcdboundingmachine.py:121) + the static
 *                             eps_schedule / grad_clipping partial args (main.py:161-172) +
 *                             the config.model routing of load_model
 *                             (/root/reference/src/model_handler.py:30-43).
 *   cmcd_layout          <->  `unflatten` of jax.flatten_util.ravel_pytree
 *                             (/root/reference/src/mcdboundingmachine.py:122,141-143): where each
 *                             leaf of (params_train, params_notrain) sits inside params_flat.
 *   cmcd_stats_merge     <->  batch_log_elbos.mean() / .var(ddof=0) (mcdboundingmachine.py:205,231)
 *                             and logsumexp(-loss) - log n (/root/reference/src/utils.py:233-235),
 *                             in a form that merges across ranks.
 *
 * Ownership: every pointer marked [device] is caller-owned device memory (e.g. the data_ptr() of
 * a contiguous torch tensor).  The library allocates no device memory and keeps no state that a
 * result depends on: what persists between calls is read-only or per host thread — cached device
 * attributes (CU count, LDS opt-in, written once), the diagnostic wave-priority override of
 * cmcd_coop.hip (read from the environment once), the thread-local error string and profile hook,
 * and the lgcp gradient's thread-local side stream and events.  Calls are re-entrant as long as each
 * concurrent call has its own `workspace` (two calls sharing a workspace must be ordered on one
 * stream).  All work is enqueued asynchronously on `stream` (a hipStream_t, may be 0); nothing in
 * cmcd_bound_forward synchronises, so it can be captured into a hipGraph.
 * Errors: 0 on success, negative cmcd_status otherwise; message via cmcd_last_error()
 * (thread-local).  Nothing throws across this boundary.
 */
#ifndef CMCD_HIP_H
#define CMCD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMCD_ABI_VERSION 3   /* 2: cmcd_adam_step[_dev] take the divergence guard (losses, n_losses, diverged)
                                3: CMCD_MODE_CAIS_UHA_SN, cmcd_layout.gamma */

typedef enum cmcd_status {
  CMCD_OK = 0,
  CMCD_ERR_BAD_ARG = -1,       /* null pointer, bad size, layout offset missing          */
  CMCD_ERR_UNSUPPORTED = -2,   /* mode / arch / target / shape not implemented           */
  CMCD_ERR_WORKSPACE = -3,     /* workspace smaller than cmcd_workspace_bytes()          */
  CMCD_ERR_HIP = -4            /* a HIP runtime call failed                               */
} cmcd_status;

/* config.boundmode plugin switch (/root/reference/src/mcd_utils.py:34-190).  The two CAIS modes and
 * the two overdamped siblings on the same skeleton (MCD_ULA = Thin et al., MCD_ULA_sn = Doucet et al.,
 * /root/reference/src/mcd_over_orig.py:6-65) exist here; every other value is CMCD_ERR_UNSUPPORTED
 * ("Mode not implemented.").  MCD_ULA has no network: pass arch = CMCD_ARCH_DDS and network layout
 * offsets of -1; eps_schedule / grad_clipping are ignored for both ULA modes, as in the reference. */
enum { CMCD_MODE_CAIS_SN = 0, CMCD_MODE_CAIS_VAR_SN = 1, CMCD_MODE_ULA = 2, CMCD_MODE_ULA_SN = 3,
       /* 2nd-order CMCD (/root/reference/src/mcd_under_lp_a_cais.py:6-115 via mcd_utils.py:174-188): state (z, rho), the
        * score network takes concat(z, rho) (built with rho_dim = dim, mcdboundingmachine.py:82-98: geffner width
        * 2 dim + emb_dim, dds first layer [2 dim + 64, 64]), eta_aux = gamma * eps, one leap-frog step per bridge.  The
        * function body fixes the cos^2 step-size schedule and the 1e2 clip of grad log p: eps_schedule / grad_clipping
        * of the descriptor are ignored for this mode. */
       CMCD_MODE_CAIS_UHA_SN = 4 };
/* config.nn_arch (/root/reference/src/nn.py:21-39) */
enum { CMCD_ARCH_GEFFNER = 0, CMCD_ARCH_DDS = 1 };
/* config.model routing (/root/reference/src/model_handler.py:30-43) */
enum { CMCD_TARGET_GMM = 0, CMCD_TARGET_FUNNEL = 1, CMCD_TARGET_MANY_GMM = 2, CMCD_TARGET_LGCP = 3 };
/* config.eps_schedule (/root/reference/src/mcd_cais.py:54-59) */
enum { CMCD_EPS_CONST = 0, CMCD_EPS_LINEAR = 1, CMCD_EPS_COS_SQ = 2 };

typedef struct cmcd_desc {
  int32_t dim;            /* params_fixed[0]                                              */
  int32_t nbridges;       /* params_fixed[1]; >= 1                                        */
  int32_t mode;           /* params_fixed[2] as CMCD_MODE_*                               */
  int32_t arch;           /* which apply_fun_sn: CMCD_ARCH_*                              */
  int32_t emb_dim;        /* geffner: config.emb_dim (net width = dim + emb_dim); dds: 64 */
  int32_t target;         /* CMCD_TARGET_*                                                */
  int32_t eps_schedule;   /* CMCD_EPS_*                                                   */
  int32_t grad_clipping;  /* 0 / 1                                                        */
  int32_t ngrid;          /* len(mgridref_y) - 1  (mcdboundingmachine.py:107-112)         */
  int32_t reserved;       /* kernel variant (testing): 0 auto, 1 wave-per-tile, 2 CU-cooperative, 3 / 4 cooperative on 16- / 8-particle
                             tiles, 5 = 4 with a wide state (d = 10) kept on the narrow-state kernel (A / B); 2nd-order mode: 4 without the
                             4-neuron tail on the last MLP wave (A / B) */
} cmcd_desc;

/* Offsets (in floats) of each leaf inside params_flat; -1 = absent for this arch.
 * Dense weights are [in, out] row-major (stax Dense / haiku Linear: x @ W + b). */
typedef struct cmcd_layout {
  int64_t vd_mean, vd_logdiag;           /* [dim] each  (vardist/diag_gauss.py:6-7)       */
  int64_t eps;                           /* scalar                                        */
  int64_t mgridref_y;                    /* [ngrid+1]                                     */
  int64_t gamma;                         /* scalar friction (MCD_CAIS_UHA_sn: eta_aux = gamma * eps,
                                            /root/reference/src/mcd_under_lp_a_cais.py:50); -1 otherwise   */
  /* geffner (/root/reference/src/nn.py:42-72), in = dim + emb_dim */
  int64_t g_emb;                         /* [nbridges, emb_dim]                           */
  int64_t g_factor;                      /* scalar factor_sn                              */
  int64_t g_w1, g_b1, g_w2, g_b2;        /* [in,in],[in] x2                               */
  int64_t g_w3, g_b3;                    /* [in,dim],[dim]                                */
  /* dds PISNet (/root/reference/src/nn_dds.py:91-164), H = 64 */
  int64_t d_phase;                       /* timestep_phase [64]                           */
  int64_t d_tw1, d_tb1, d_tw2, d_tb2;    /* time coder [128,64],[64],[64,64],[64]         */
  int64_t d_sw1, d_sb1;                  /* [dim+64,64],[64]                              */
  int64_t d_sw2, d_sb2;                  /* [64,64],[64]                                  */
  int64_t d_sw3, d_sb3;                  /* LinearZero [64,dim],[dim]                     */
} cmcd_layout;

/* out_stats: 5 doubles, the mergeable batch statistics of the per-particle losses l_n:
 *   [0] number of finite l_n   [1] sum l_n   [2] sum l_n^2
 *   [3] M = max_n(-l_n)        [4] sum_n exp(-l_n - M)
 * +inf losses are legal (many_gmm floor, /root/reference/src/model_handler.py:279-280) and make
 * [1],[2] +inf exactly like the reference's mean/var; NaN anywhere means "diverged"
 * (/root/reference/src/opt.py:122). */
#define CMCD_NSTATS 5

int cmcd_version(void);
const char* cmcd_last_error(void);

/* Bytes of [device] scratch cmcd_bound_forward needs for n particles (0 on bad desc). */
int64_t cmcd_workspace_bytes(const cmcd_desc* desc, int64_t n);

/* Number of floats of target constants expected for desc->target:
 *   gmm: 0; funnel: 0; many_gmm: 1 + 2*n_mixes = {scale, means[n_mixes,2]} (n_target tells
 *   n_mixes); lgcp: dim*dim + dim + 3 = {Kinv[dim,dim], counts[dim], mu0, a, lognorm}. */
int64_t cmcd_target_floats(const cmcd_desc* desc, int32_t n_mixes);

/* One forward evaluation of the bound for n particles:
 *   seeds[n] int32 [device]  ->  out_loss[n] = -w_n, out_z[n*dim] = z_K  [device, float32],
 *   out_stats[5] [device, float64].  params[n_params] float32 [device] is params_flat.  */
int cmcd_bound_forward(const cmcd_desc* desc, const cmcd_layout* layout,
                       const int32_t* seeds, int64_t n,
                       const float* params, int64_t n_params,
                       const float* target_consts, int64_t n_target,
                       void* workspace, int64_t workspace_bytes,
                       float* out_loss, float* out_z, double* out_stats,
                       void* stream);

/* Evaluation loops on FIXED parameters (the reference's `opt.sample` calls its jitted loss_fn n_input_dist_seeds = 30 times
 * with the same params_flat, /root/reference/src/opt.py:185-190; XLA keeps nothing between those calls either, but its
 * executable has no per-call table-building stage): same arguments and results as cmcd_bound_forward, but the per-call PREP
 * launch (the beta / eps schedule, the time path of the score network folded into per-bridge first-layer biases, the
 * operand packing of the weights: everything that depends on params_flat and not on the particles) is skipped.
 * CONTRACT: `workspace` was last used by a cmcd_bound_forward / cmcd_bound_forward_prepared call with the SAME desc, layout,
 * n, params CONTENTS and target constants, and nothing wrote into it since.  The library cannot check this (it keeps no
 * state and never reads params back to the host): the caller owns the invalidation — the Python mirror takes this entry point
 * only inside an explicit `fixed_parameters()` context, where it keys the tables on (workspace, the parameter tensor OBJECT,
 * its data_ptr() and version counter, target constants, desc, layout, n) and bumps the version counter wherever it updates
 * parameters through a raw pointer (cmcd_adam_step).  On the d = 1600 (lgcp) launch sequences the prepared
 * form skips the schedule / bias-table launches and the re-packing of the weights (the per-call zeroing of the operand
 * buffers stays); the 2nd-order lgcp sequence ignores the hint and prepares every call. */
int cmcd_bound_forward_prepared(const cmcd_desc* desc, const cmcd_layout* lay,
                                const int32_t* seeds, int64_t n,
                                const float* params, int64_t n_params,
                                const float* target_consts, int64_t n_target,
                                void* workspace, int64_t workspace_bytes,
                                float* out_loss, float* out_z, double* out_stats,
                                void* stream);

/* ---- The reverse-time chain: draws from the TARGET pushed through the backward kernels of the sampler.  No analogue in the
 * reference, which runs its chain from q only; the arithmetic is its forward chain's (/root/reference/src/mcd_cais.py:46-89,
 * mcd_cais_var.py, mcd_over_orig.py:22-56, mcdboundingmachine.py:126-179) walked the other way, restated in float64 NumPy in
 * tests/test_gpu_reverse.py.  With the schedules beta_i, eps_i, the clip rule, the network s(., i) and q of cmcd_bound_forward
 * for the same (desc, layout, params) — the same prep tables — and sigma_i = sqrt(2 eps_i), particle p runs
 *   z_K = x_p;  w = log p(z_K)
 *   for i = K-1 .. 0:   m_b = z_{i+1} - eps_i gradU(z_{i+1}, beta_i) + eps_i s(z_{i+1}, j)     j = i + 1 (MCD_CAIS_sn, MCD_CAIS_var_sn),
 *                                                                         j = i (MCD_ULA_sn), no network term (MCD_ULA)
 *                       z_i = m_b + sigma_i xi_r,  r = K-1-i
 *                       m_f = z_i - eps_i gradU(z_i, beta_i) - eps_i s(z_i, i)                 (network term: the CAIS modes only)
 *                       w  += log N(z_i; m_b, sigma_i) - log N(z_{i+1}; m_f, sigma_i)
 *   w -= log q(z_0)
 * so w is the functional cmcd_bound_forward returns as -loss, on a path drawn from p(z_K) prod B_i.  E[w] >= ln Z (the EUBO:
 * with the forward call's ELBO it brackets ln Z), and exp(-w) are the importance weights of the reverse estimate of 1 / Z.
 * xi_r comes from the forward call's key chain without its first key: (_, gen) = split(PRNGKey(seed)); (C, _) = split(gen);
 * gen_0 = second(split(C)); step r: (G, H) = split(gen), xi_r = normal(G, (dim,)), gen = second(split(H)).
 *   x[n*dim] float32 [device], seeds[n] int32 [device]  ->  out_w[n], out_z0[n*dim] = z_0 [device, float32],
 *   out_stats[5] [device, float64] = the statistics above over l := w (they merge with cmcd_stats_merge[_device]):
 *   EUBO = out_stats[1] / n;  reverse ln Z = -(out_stats[3] + log out_stats[4] - log n).
 * A particle whose x row holds a non-finite entry, or whose w comes out NaN, gets w = +inf (weight 0; its z_0 row is
 * meaningless): the EUBO of such a batch is +inf, never NaN.
 * Ownership, stream, no-host-sync and capture rules as cmcd_bound_forward; workspace of cmcd_reverse_workspace_bytes (0 where
 * the call is unsupported).  One kernel form (one wave per 16-particle tile) for the overdamped modes on gmm, funnel (dim 10)
 * and many_gmm with the nets cmcd_bound_forward's wave-per-tile kernel is built for; lgcp and other widths:
 * CMCD_ERR_UNSUPPORTED, and so is MCD_CAIS_UHA_sn here: its reverse chain carries a momentum and is cmcd_bound_reverse_uha, below. */
int64_t cmcd_reverse_workspace_bytes(const cmcd_desc* desc, int64_t n);
int cmcd_bound_reverse(const cmcd_desc* desc, const cmcd_layout* layout,
                       const int32_t* seeds, const float* x, int64_t n,
                       const float* params, int64_t n_params,
                       const float* target_consts, int64_t n_target,
                       void* workspace, int64_t workspace_bytes,
                       float* out_w, float* out_z0, double* out_stats,
                       void* stream);

/* ---- Resumable segments of the forward chain: bridges [k0, k1) from a caller-supplied particle state, so that the weights can
 * be examined and the particles resampled BETWEEN bridges (sequential Monte Carlo over the annealing path; the Python driver is
 * cmcd_amd.smc).  No analogue in the reference, which runs its chain from q to bridge K in one piece; the arithmetic is the
 * forward call's, cut at a bridge, restated in float64 NumPy in tests/smc_restatement.py.  With the schedules beta_i, eps_i, the
 * clip rule, the network s(., i) and q of cmcd_bound_forward for the same (desc, layout, params) — the same prep tables —
 * particle p runs
 *   k0 == 0:  key chain and z_0 exactly as cmcd_bound_forward;  wpath = -log q(z_0);  gen = gen_0
 *   k0  > 0:  z = z_inout[p], wpath = wpath_inout[p], gen = key_inout[p]      (uint32[2]: the forward chain's gen_k0)
 *   for i = k0 .. k1-1:  the forward call's step i, unchanged:  z' = m_f(z, i) + sigma_i xi_i with xi_i = normal(first(split(gen)));
 *                        wpath += log B_i(z | z') - log F_i(z' | z);  z <- z';  gen <- second(split(second(split(gen))))
 *   lg = log gamma_k1(z):  gamma_K = p;  0 < k < K:  log gamma_k = beta_{k-1} log p + (1 - beta_{k-1}) log q
 *   out:  z_inout[p] = z, wpath_inout[p] = wpath, key_inout[p] = gen_k1, out_lg[p] = lg;
 *         out_stats[5] = the statistics of cmcd_bound_forward over l := -(wpath + lg).
 * Why beta_{k-1}: step k-1 uses beta_{k-1} at both of its ends, so with a zero network wpath + lg telescopes to the plain AIS
 * weight of particles that target pi_{beta_{k-1}} = p^beta q^(1 - beta).  log p = -inf (the many_gmm floor) gives lg = -inf
 * whatever beta is, never 0 * inf; a NaN stays NaN (the divergence signal, as in the forward call).  At k1 == nbridges,
 * -(wpath + lg) is the loss cmcd_bound_forward returns (same arithmetic; its wave-per-tile kernel evaluates the 132-wide net in
 * another order, so the last bits may differ).  wpath is carried WITHOUT the gamma term: segments [0, k) then [k, K) need no
 * cancellation and return the bits of the single segment [0, K) in z, wpath, lg and the key — the kernel is one
 * runtime-bounded loop with a single evaluation site, so the evaluation at a cut is the same machine code in both segments.
 * It is also evaluated by both: one extra evaluation (grad log p, grad log q, the network) per cut.
 * The state is read and overwritten in place (each particle by its own lanes only).  Keys belong to the particle SLOT: a
 * caller that resamples z between segments leaves key_inout alone, so that two offspring of one ancestor draw different noise.
 *   0 <= k0 < k1 <= nbridges, else CMCD_ERR_BAD_ARG;  seeds[n] int32 [device] is read when k0 == 0 (null there:
 *   CMCD_ERR_BAD_ARG) and may be null otherwise.  z_inout[n*dim], wpath_inout[n], out_lg[n] float32, key_inout[n*2] uint32,
 *   out_stats[5] float64, all [device].
 * Ownership, stream, no-host-sync and capture rules as cmcd_bound_forward; workspace of cmcd_segment_workspace_bytes (0 where
 * the call is unsupported).  Every call runs the prep launch (there is no prepared-table form).  One kernel form (one wave per
 * 16-particle tile) for the four overdamped modes on gmm, funnel (dim 10) and many_gmm with the nets of cmcd_bound_reverse
 * (dds 64; geffner on 2 / 4 / 9 neuron tiles, funnel 4 / 9); MCD_CAIS_UHA_sn, lgcp and other widths: CMCD_ERR_UNSUPPORTED. */
int64_t cmcd_segment_workspace_bytes(const cmcd_desc* desc, int64_t n);
int cmcd_bound_segment(const cmcd_desc* desc, const cmcd_layout* layout, int32_t k0, int32_t k1,
                       const int32_t* seeds /* k0 == 0; else nullable */, int64_t n,
                       const float* params, int64_t n_params,
                       const float* target_consts, int64_t n_target,
                       void* workspace, int64_t workspace_bytes,
                       float* z_inout /*[n*dim]*/, float* wpath_inout /*[n]*/, uint32_t* key_inout /*[n*2]*/,
                       float* out_lg /*[n]*/, double* out_stats /*[5]*/, void* stream);

/* ---- The same for MCD_CAIS_UHA_sn (2nd-order CMCD), whose particle state carries the momentum: bridges [k0, k1) from
 * (z, rho, wpath, key); the Python driver is cmcd_amd.smc_uha, the float64 restatement tests/smc_uha_restatement.py.
 * Schedules (cos^2, always), the clip of grad log p at 1e2, the network s([z; rho], i) and q are those of cmcd_bound_forward
 * for the same (desc, layout, params) in mode CMCD_MODE_CAIS_UHA_SN — the same prep tables.  With eta_i = gamma eps_i,
 * sigma_i = sqrt(2 eta_i) and gU(z, b) = -(b clip(grad log p(z), +-1e2) + (1 - b) grad log q(z)), particle p runs
 *   k0 == 0:  (A, B) = split(PRNGKey(seed));  z_0 = mean + std normal(A);  C = first(split(B));  (R, G') = split(C);
 *             rho_0 = normal(R);  gen_0 = second(split(G'))   (one more split in front of gen_0 than the overdamped chain);
 *             wpath = -log q(z_0) - log N(rho_0; 0, I)
 *   k0  > 0:  z = z_inout[p], rho = rho_inout[p], wpath = wpath_inout[p], gen = key_inout[p]   (the forward chain's gen_k0)
 *   for i = k0 .. k1-1, the forward call's bridge i, unchanged:
 *             m_f = rho (1 - eta_i) - 2 eta_i s([z; rho], i);   rho' = m_f + sigma_i xi_i,  xi_i = normal(first(split(gen)))
 *             rho'' = rho' - eps_i gU(z, beta_i) / 2;  z' = z + eps_i rho'';  rho_new = rho'' - eps_i gU(z', beta_i) / 2
 *             m_b = rho' (1 - eta_i) + 2 eta_i s([z; rho'], i)                       (the old z, the same index i)
 *             wpath += log N(rho; m_b, sigma_i) - log N(rho'; m_f, sigma_i);   (z, rho) <- (z', rho_new);
 *             gen <- second(split(second(split(gen))))
 *   lg = log gamma_k1(z) + log N(rho; 0, I):  gamma_K = p;  0 < k < K:  log gamma_k = beta_{k-1} log p + (1 - beta_{k-1}) log q
 *             (step k-1 uses beta_{k-1} at both leap-frog ends, as the overdamped step does at both of its kernels)
 *   out:  z_inout[p] = z, rho_inout[p] = rho, wpath_inout[p] = wpath, key_inout[p] = gen_k1, out_lg[p] = lg;
 *         out_stats[5] = the statistics of cmcd_bound_forward over l := -(wpath + lg).
 * log p = -inf (the many_gmm floor) gives lg = -inf whatever beta and rho are, never 0 * inf; a NaN stays NaN.  The momentum's
 * density is part of lg on purpose: -(wpath + lg) is the loss of a chain stopped at k1 (at k1 == nbridges the loss
 * cmcd_bound_forward returns); the leap-frog is a volume-preserving bijection of (z, rho), so exp(wpath + lg) is a proper
 * weight for gamma_k1(z) N(rho; 0, I) whatever the network is; and a resampling stage restarts its offspring with
 * wpath = -lg[ancestor] exactly as for the overdamped state.  A caller that resamples moves z AND rho with the same
 * ancestors and leaves key_inout alone (keys belong to the slot).
 * The kernel is ONE runtime-bounded rotated loop m = k0 .. k1 with a single site that evaluates (log p, grad log p,
 * grad log q) at z_m: for m > k0 it closes step m - 1 (rho = rho'' - eps_{m-1} ub / 2), for m < k1 it opens step m, at
 * m == k1 it forms lg; the two network evaluations of a step stay inside the step.  So [0, k) then [k, K) returns the BITS
 * of [0, K) in z, rho, wpath, lg and the key, at the price of one extra target evaluation per cut.
 *   0 <= k0 < k1 <= nbridges, else CMCD_ERR_BAD_ARG;  seeds[n] int32 [device] is read when k0 == 0 (null there:
 *   CMCD_ERR_BAD_ARG) and may be null otherwise.  z_inout[n*dim], rho_inout[n*dim], wpath_inout[n], out_lg[n] float32,
 *   key_inout[n*2] uint32, out_stats[5] float64, all [device].
 * Ownership, stream, no-host-sync and capture rules as cmcd_bound_forward; workspace of cmcd_segment_uha_workspace_bytes (0
 * where the call is unsupported).  Every call runs the prep launch.  One kernel form (one wave per 16-particle tile) on gmm,
 * funnel (dim 10) and many_gmm with the nets of the forward call's wave-per-tile 2nd-order kernel (dds 64; geffner on 2 / 4 /
 * 5 / 9 neuron tiles); the overdamped modes (they have cmcd_bound_segment), lgcp and other widths: CMCD_ERR_UNSUPPORTED.
 * No cooperative form.  (LDVI and the UHA boundmode have segment calls of their own, cmcd_bound_segment_ldvi and
 * cmcd_bound_segment_hais below.  The reverse-time chain of this mode: cmcd_bound_reverse_uha.) */
int64_t cmcd_segment_uha_workspace_bytes(const cmcd_desc* desc, int64_t n);
int cmcd_bound_segment_uha(const cmcd_desc* desc, const cmcd_layout* layout, int32_t k0, int32_t k1,
                           const int32_t* seeds /* k0 == 0; else nullable */, int64_t n,
                           const float* params, int64_t n_params,
                           const float* target_consts, int64_t n_target,
                           void* workspace, int64_t workspace_bytes,
                           float* z_inout /*[n*dim]*/, float* rho_inout /*[n*dim]*/, float* wpath_inout /*[n]*/,
                           uint32_t* key_inout /*[n*2]*/, float* out_lg /*[n]*/, double* out_stats /*[5]*/, void* stream);

/* ---- The reverse-time chain of MCD_CAIS_UHA_sn (2nd-order CMCD): draws from the TARGET, a fresh momentum, and then the backward
 * momentum kernels and the INVERTED leap-frogs of the sampler; cmcd_bound_reverse for the mode it refuses.  The Python mirror is
 * cmcd_amd.reverse_uha, the float64 restatement tests/reverse_uha_restatement.py.  No analogue in the reference; the arithmetic
 * is its forward chain's (mcd_under_lp_a_cais.py:41-113, mcdboundingmachine.py:126-179) walked the other way.  Schedules (cos^2,
 * always), the clip of grad log p at 1e2 (always), gamma, the network s([z; rho], i) and q are those of cmcd_bound_forward for
 * the same (desc, layout, params) in mode CMCD_MODE_CAIS_UHA_SN — the same prep tables.  With eta_i = gamma eps_i,
 * sigma_i = sqrt(2 eta_i) and gU(z, b) = -(b clip(grad log p(z), +-1e2) + (1 - b) grad log q(z)), particle p runs
 *   z_K = x_p;  rho_K = normal(R);  w = log p(z_K) + log N(rho_K; 0, I)
 *   for i = K-1 .. 0:
 *             rho'' = rho_{i+1} + eps_i gU(z_{i+1}, beta_i) / 2        (the leap-frog of bridge i, inverted: undo the second
 *             z_i   = z_{i+1} - eps_i rho''                              half-kick, the drift, then the first half-kick)
 *             rho'  = rho'' + eps_i gU(z_i, beta_i) / 2
 *             m_b   = rho' (1 - eta_i) + 2 eta_i s([z_i; rho'], i)      (backward kernel: z_i, the SAME index i)
 *             rho_i = m_b + sigma_i xi_r,  r = K-1-i
 *             m_f   = rho_i (1 - eta_i) - 2 eta_i s([z_i; rho_i], i)
 *             w    += log N(rho_i; m_b, sigma_i) - log N(rho'; m_f, sigma_i)
 *   w -= log q(z_0) + log N(rho_0; 0, I)
 * so w is the functional cmcd_bound_forward returns as -loss in this mode, on a path drawn from p(z_K) N(rho_K) prod B_i.  The
 * leap-frog is a volume-preserving bijection: no Jacobian term.  E[w] >= ln Z (the EUBO: with the forward call's ELBO it
 * brackets ln Z), and exp(-w) are the importance weights of the reverse estimate of 1 / Z.  The densities are evaluated at the
 * z_i the inverted leap-frog produces; whether a float32 forward leap-frog from (z_i, rho') lands on (z_{i+1}, rho_{i+1})
 * again does not enter w.
 * Key chain: the forward call's for this mode without its first draw.  (_, B) = split(PRNGKey(seed));  C = first(split(B));
 * (R, G') = split(C);  rho_K = normal(R, (dim,)) — the key the forward chain spends on rho_0;  gen_0 = second(split(G'));
 * reverse step r: (G, H) = split(gen), xi_r = normal(G, (dim,)), gen = second(split(H)).
 *   x[n*dim] float32 [device], seeds[n] int32 [device]  ->  out_w[n], out_z0[n*dim] = z_0, out_rho0[n*dim] = rho_0
 *   [device, float32], out_stats[5] [device, float64] = the statistics of cmcd_bound_forward over l := w:
 *   EUBO = out_stats[1] / n;  reverse ln Z = -(out_stats[3] + log out_stats[4] - log n).
 * A particle whose x row holds a non-finite entry, or whose w comes out NaN, gets w = +inf (weight 0; its z_0 and rho_0 rows
 * are meaningless): the EUBO of such a batch is +inf, never NaN; the other particles of its tile keep their bits.
 * The kernel is ONE rotated loop m = K .. 0 with a single site that evaluates (log p, grad log p, grad log q) at z_m: for
 * m < K it closes the inverse leap-frog of bridge m, and the two network evaluations (same z_m, same row m: the z part of the
 * first layer is formed once) and both densities follow; for m > 0 it opens bridge m - 1; at m == K it gives log p(z_K).
 * K + 1 target evaluations and 2 K network evaluations, the forward kernel's count.
 * Null seeds, x or output pointer, n < 1: CMCD_ERR_BAD_ARG; a short or misaligned workspace: CMCD_ERR_WORKSPACE.
 * Ownership, stream, no-host-sync and capture rules as cmcd_bound_forward; workspace of cmcd_reverse_uha_workspace_bytes
 * (= cmcd_workspace_bytes; 0 where the call is unsupported).  Every call runs the prep launch (there is no prepared-table
 * form).  One kernel form (one wave per 16-particle tile) on gmm, funnel (dim 10) and many_gmm with the nets of the forward
 * call's wave-per-tile 2nd-order kernel (dds 64; geffner on 2 / 4 / 5 / 9 neuron tiles); the overdamped modes (they have
 * cmcd_bound_reverse), lgcp and other widths: CMCD_ERR_UNSUPPORTED, decided on the host before any device work.
 * No cooperative form.  LDVI and the UHA boundmode have reverse chains of their own: cmcd_bound_reverse_ldvi and
 * cmcd_bound_reverse_hais, below; this call keeps refusing them. */
int64_t cmcd_reverse_uha_workspace_bytes(const cmcd_desc* desc, int64_t n);
int cmcd_bound_reverse_uha(const cmcd_desc* desc, const cmcd_layout* layout,
                           const int32_t* seeds, const float* x, int64_t n,
                           const float* params, int64_t n_params,
                           const float* target_consts, int64_t n_target,
                           void* workspace, int64_t workspace_bytes,
                           float* out_w /*[n]*/, float* out_z0 /*[n*dim]*/, float* out_rho0 /*[n*dim]*/,
                           double* out_stats /*[5]*/, void* stream);

/* (Measurement and diagnostic hooks — kernel-time events, the PRNG capture of the parity tests, the probes' switches — are NOT
 * part of this boundary: they are declared in include/cmcd_hip_diag.h and compiled out of the library by
 * -DCMCD_NO_DIAG_HOOKS; a deployment binds nothing of them.) */

/* ---- VarGrad gradient ("compute_log_var_grad"): d/d params_flat of compute_bound_var
 * (/root/reference/src/main.py:161-176 takes jax.grad of it; /root/reference/src/mcd_cais_var.py:59,79
 * detach z, which makes the gradient local per bridge).  Two calls after a cmcd_bound_forward on the
 * same seeds / params:
 *   cmcd_vargrad_weights  omega[n] = d var / d w_n = -(2/N)(l_n - mean l) from loss[n] and the (merged,
 *                         for multi-GPU) statistics; n_total = global particle count.  All zero while
 *                         |var| > 1e7: the bound is clip(var, +-1e7) (mcdboundingmachine.py:231).
 *   cmcd_bound_var_grad   grad[n_params] (overwritten; zeros for leaves without gradient) =
 *                         sum_n omega_n d w_n / d params_flat.  Across ranks: all-reduce(sum) of grad.
 * MCD_CAIS_var_sn only; kernel instances exist for the BASELINE nets (dds 64; geffner widths up to 144 on the
 * 2-d targets, 64 on funnel) and lgcp (geffner, any width: the launch-sequence reverse sweep with z detached —
 * through cmcd_bound_var_forward + cmcd_bound_var_grad_kept only); CMCD_ERR_UNSUPPORTED otherwise. */
int64_t cmcd_grad_workspace_bytes(const cmcd_desc* desc, int64_t n);
int cmcd_vargrad_weights(const float* loss, const double* stats, int64_t n, int64_t n_total, float* omega,
                         void* stream);
int cmcd_bound_var_grad(const cmcd_desc* desc, const cmcd_layout* layout, const int32_t* seeds, int64_t n,
                        const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                        const float* omega, void* workspace, int64_t workspace_bytes, float* grad, void* stream);
/* The same two steps without running the chain twice: cmcd_bound_var_forward is cmcd_bound_forward on the
 * GRADIENT workspace (cmcd_grad_workspace_bytes) and leaves the per-call tables — and, for batches small
 * enough for the work-item gradient path, the trajectory z_0..z_K (lgcp: also every evaluation's activations, which the
 * reverse launch sequence then reads instead of recomputing them) — there; cmcd_bound_var_grad_kept then
 * needs the same desc / seeds / params / workspace, untouched in between (weights from
 * cmcd_vargrad_weights as before). */
int cmcd_bound_var_forward(const cmcd_desc* desc, const cmcd_layout* layout, const int32_t* seeds, int64_t n,
                           const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                           void* workspace, int64_t workspace_bytes, float* out_loss, float* out_z,
                           double* out_stats, void* stream);
int cmcd_bound_var_grad_kept(const cmcd_desc* desc, const cmcd_layout* layout, const int32_t* seeds, int64_t n,
                             const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                             const float* omega, void* workspace, int64_t workspace_bytes, float* grad, void* stream);

/* ---- Reparameterised gradient of the mean bound: what jax.value_and_grad(compute_bound, 1, has_aux=True)
 * returns for MCD_CAIS_sn (/root/reference/src/main.py:174-176 over mcdboundingmachine.py:183-205 and
 * mcd_cais.py:46-89 — no stop_gradient, so the gradient flows back through every z_i: the net's input
 * Jacobian, the Hessians of log p and log q, and the step-size / beta schedules).
 * One call = forward (losses, z_K, statistics as cmcd_bound_forward; the trajectory z_0..z_K is kept in
 * the workspace) + reverse sweep.  grad[n_params] (overwritten) = omega * sum_n d loss_n / d params_flat;
 * omega = d value / d loss_n = 1 / N_total (across ranks: all-reduce(sum) of grad).
 * Also MCD_ULA_sn and MCD_ULA (/root/reference/src/mcd_over_orig.py), on every target.
 * Targets gmm / funnel / many_gmm with the BASELINE nets (dds 64; geffner widths up to 144 on the 2-d targets,
 * 64 on funnel), and lgcp (geffner, any width: launch-sequence reverse sweep); CMCD_ERR_UNSUPPORTED otherwise.
 * Repeated calls with the same arguments return the same bits (r04): every sum over particles is taken in a fixed order
 * — per-tile slots + a reduction launch; the workspace holds the slots — for gmm / funnel / many_gmm in every mode, up to a
 * slot table of 1 GB (about 245 000 particles at K = 256 with the 64-wide dds net); above it the overdamped modes'
 * bias-row and schedule sums fall back to float atomics and the last bits may differ from call to call.  (The
 * reference's own gradients are XLA reductions: deterministic on one device.) */
/* Workspace growth to plan for: beside the kept trajectory ((K + 1) n dim floats; 3 K + 2 rows of n dim for MCD_CAIS_UHA_sn) the
 * fixed-order sums keep one slot row per (16-particle tile, evaluation): K HP (2 | 4) / 16 floats per particle.  The overdamped
 * modes cap that table at 1 GB and fall back to atomics above it (see above); MCD_CAIS_UHA_sn has NO cap and no fallback — with the
 * 144-wide geffner net and K = 256 it is ~37 KB per particle: 0.6 GB at n = 16 000, 2.4 GB at n = 65 536 on top of the trajectory.
 * Query this function and split larger 2nd-order batches on the caller's side (gradients of particle batches add). */
int64_t cmcd_bound_grad_workspace_bytes(const cmcd_desc* desc, int64_t n);
int cmcd_bound_grad(const cmcd_desc* desc, const cmcd_layout* layout, const int32_t* seeds, int64_t n,
                    const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                    float omega, void* workspace, int64_t workspace_bytes,
                    float* out_loss, float* out_z, double* out_stats, float* grad, void* stream);

/* ---- Mean-field VI ("pretrain_mfvi"): the reference's plain bounding machine with nbridges = 0
 * (/root/reference/src/boundingmachine.py:73-111, bm.compute_bound :114-118), which
 * /root/reference/src/main.py:82-109 optimises with trainable = ("vd",) to obtain the q every CMCD run
 * starts from.  Per seed: z = mean + exp(logdiag) * normal(first(split(PRNGKey(seed)))) (the same z_0 as
 * cmcd_bound_forward draws), loss = log q(z) - log p(z).  out_loss / out_z / out_stats as cmcd_bound_forward.
 * grad (nullable: forward only) [n_params], overwritten: omega * sum_n d loss_n / d {vd.mean, vd.logdiag}
 * under the reparameterisation, zeros elsewhere; omega = 1 / N_total.
 * Targets: gmm, many_gmm (dim 2), funnel (dim 10), lgcp (dim = m^2). */
int64_t cmcd_mfvi_workspace_bytes(int32_t target, int32_t dim, int64_t n);
int cmcd_mfvi_bound_grad(int32_t target, int32_t dim, int64_t off_vd_mean, int64_t off_vd_logdiag,
                         const int32_t* seeds, int64_t n, const float* params, int64_t n_params,
                         const float* target_consts, int64_t n_target, float omega,
                         void* workspace, int64_t workspace_bytes,
                         float* out_loss, float* out_z, double* out_stats, float* grad, void* stream);

/* ---- UHA, Hamiltonian AIS: the reference's plain bounding machine with nbridges >= 1 (config.boundmode = "UHA",
 * /root/reference/src/boundingmachine.py:73-111 -> ais_utils.py:7-69 -> momdist.py:13-28), bound and reparameterised gradient.
 * No network.  Per seed, with s = exp(md), L = lfsteps, gU(z, b) = -(b grad log p(z) + (1 - b) grad log q(z)) (no clip):
 *   (A, B) = split(PRNGKey(seed));  z = mean + exp(logdiag) normal(A);  w = -log q(z)
 *   C = first(split(B));  (R, G') = split(C);  rho_prev = s normal(R);  gen = second(split(G'))
 *   beta = interp(target_x, gridref_x, [0, cumsum(mgridref_y) / sum(mgridref_y)])
 *   for i = 0 .. nbridges-1:
 *     (G, H) = split(gen);  xi = normal(G);  gen = second(split(H))
 *     rho = eta rho_prev + sqrt(1 - eta^2) s xi
 *     r = rho - eps/2 gU(z, beta_i);  z += eps r / s^2;  (L-1) times: r -= eps gU(z, beta_i), z += eps r / s^2;
 *     r -= eps/2 gU(z, beta_i);  w += log N(r; 0, s) - log N(rho; 0, s);  rho_prev = r
 *   w += log p(z);  loss = -w
 * (eps is the scalar parameter, constant over the bridges; no initial or final momentum term; delta_H is not produced).
 * out_loss / out_z / out_stats as cmcd_bound_forward.  grad (nullable: forward only) [n_params], overwritten:
 * omega * sum_n d loss_n / d {vd.mean, vd.logdiag, eps, eta, md, mgridref_y}, zeros elsewhere; omega = 1 / N_total.  The forward
 * call and the gradient call return the same loss bits, repeated calls the same gradient bits (per-tile slots summed in a
 * fixed order, no floating-point atomics).  A gradient call keeps (nbridges L + 1) + (2 nbridges + 1) rows of n dim floats in the
 * workspace.  Ownership, stream, no-host-sync and capture rules as cmcd_bound_forward.
 * Targets: gmm, many_gmm (dim 2), funnel (dim 10); lgcp (it has entry points of its own, cmcd_hais_lgcp_bound_grad below) and
 * every other (target, dim): CMCD_ERR_UNSUPPORTED, and 0 from the size query.  nbridges <= 4096, ngrid <= 1024, eta < 1. */
typedef struct cmcd_hais_layout {          /* offsets (in floats) of the leaves inside params_flat */
  int64_t vd_mean, vd_logdiag;             /* [dim] each                                      */
  int64_t eps, eta;                        /* scalars                                         */
  int64_t md;                              /* [dim]  log scales of the momentum distribution  */
  int64_t mgridref_y;                      /* [ngrid+1]                                       */
  int64_t gridref_x;                       /* [ngrid+2]                                       */
  int64_t target_x;                        /* [nbridges]                                      */
  int64_t ngrid;                           /* len(mgridref_y) - 1 (a count, not an offset)    */
} cmcd_hais_layout;
int64_t cmcd_hais_workspace_bytes(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, int64_t n, int32_t with_grad);
int cmcd_hais_bound_grad(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout* layout,
                         const int32_t* seeds, int64_t n, const float* params, int64_t n_params,
                         const float* target_consts, int64_t n_target, float omega,
                         void* workspace, int64_t workspace_bytes,
                         float* out_loss, float* out_z, double* out_stats, float* grad /* nullable: forward only */, void* stream);

/* ---- UHA on lgcp (dim = 1600): the arithmetic of the UHA block above, unchanged (key chain, refresh, opening half kick,
 * L - 1 full kicks, closing half kick, weight term, nbridges L + 1 target evaluations, no clip, eps the scalar leaf, betas from
 * mgridref_y), on the target log p(z) = counts . z - a sum e^z - 1/2 (z - mu0)^T K^-1 (z - mu0) + lognorm, as a launch sequence
 * (cmcd_amd/csrc/cmcd_hais_lgcp.hip): one launch per target evaluation, the product with K^-1 on the matrix cores and the whole
 * leap-frog step in its epilogue; the reverse sweep is again one launch and one product per evaluation.
 * target_consts = {Kinv[dim, dim], counts[dim], mu0, a, lognorm} (cmcd_amd.lgcp.lgcp_constants), 16-byte aligned; n_target must be
 * dim * dim + dim + 3.  layout, seeds, params, omega, out_loss / out_z / out_stats and grad as cmcd_hais_bound_grad: grad (nullable:
 * forward only) [n_params], overwritten: omega * sum_n d loss_n / d {vd.mean, vd.logdiag, eps, eta, md, mgridref_y}, zeros
 * elsewhere.  The forward call and the gradient call return the same loss and z bits, repeated calls the same gradient bits
 * (slots summed in a fixed order, no floating-point atomics).  Every launch goes on `stream`; no host synchronisation, no
 * allocation, capturable.  Workspace per particle: 5 rows of dim floats, 2 nbridges + 2 key words and 100 slots; a gradient call
 * additionally keeps 2 (nbridges L + 1) + 2 nbridges + 1 rows of n dim floats (the position and its product with K^-1 of every
 * evaluation, the refreshed momentum of every bridge, the momentum between the bridges) and 8 rows of sweep state.
 * dim = 1600 only; every other dim: CMCD_ERR_UNSUPPORTED, and 0 from the size query (with the error text set).
 * nbridges <= 4096, nbridges * lfsteps <= 2^24, n <= 2^20 (CMCD_ERR_UNSUPPORTED above), ngrid <= 1024, eta < 1. */
int64_t cmcd_hais_lgcp_workspace_bytes(int32_t dim, int32_t nbridges, int32_t lfsteps, int64_t n, int32_t with_grad);
int cmcd_hais_lgcp_bound_grad(int32_t dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout* layout,
                              const int32_t* seeds, int64_t n, const float* params, int64_t n_params,
                              const float* target_consts, int64_t n_target, float omega,
                              void* workspace, int64_t workspace_bytes,
                              float* out_loss, float* out_z, double* out_stats, float* grad /* nullable: forward only */, void* stream);

/* ---- LDVI: config.boundmode = "MCD_U_a-lp-sn" (use_net = 1) and its network-free sibling "MCD_U_a-lp" (use_net = 0),
 * /root/reference/src/mcd_under_lp_a.py:6-87 reached through mcd_utils.py:83-120 from mcdboundingmachine.py:126-179; bound and
 * reparameterised gradient.  Per seed, with eta = gamma eps, sigma = sqrt(2 eta), gU(z, b) = -(b grad log p(z) +
 * (1 - b) grad log q(z)) (plain jax.grad(U): no clip) and eps the scalar parameter, constant over the bridges:
 *   (A, B) = split(PRNGKey(seed));  z = mean + exp(logdiag) normal(A);  w = -log q(z)           mcdboundingmachine.py:151-157
 *   C = first(split(B));  (R, G') = split(C);  rho = normal(R);  w -= log N(rho; 0, 1)          mcd_under_lp_a.py:66-71
 *   gen = second(split(G'));  beta = interp(target_x, gridref_x, [0, cumsum(mgridref_y) / sum(mgridref_y)])
 *   for i = 0 .. nbridges-1:
 *     (G, H) = split(gen);  n_i = normal(G);  gen = second(split(H))                             :32,60
 *     m_f = rho (1 - eta);  rho' = m_f + sigma n_i                                               :28-33
 *     rho'' = rho' - eps/2 gU(z, beta_i);  z' = z + eps rho'';  rho_new = rho'' - eps/2 gU(z', beta_i)   :35-37
 *     m_b = rho' (1 - eta) + 2 eta s([z; rho'], i)      (the old z; use_net = 0: no s term)      :41-51
 *     w += log N(rho; m_b, sigma) - log N(rho'; m_f, sigma);  (z, rho) = (z', rho_new)           :54-61
 *   w += log N(rho; 0, 1) + log p(z);  loss = -w                                                 :85, mcdboundingmachine.py:178
 * The network is the one of CMCD_MODE_CAIS_UHA_SN (built with rho_dim = dim: geffner width 2 dim + emb_dim); there is no
 * network in the forward kernel and one evaluation per bridge.  grad log p(z') closes bridge i and opens bridge i + 1:
 * nbridges + 1 target evaluations per particle.  many_gmm's floor: grad log p = 0 where floored, loss = +inf when z_K is.
 * desc: dim, nbridges, arch, emb_dim, target, ngrid are read; mode, eps_schedule, grad_clipping and reserved are IGNORED (the
 * function body has neither a schedule nor a clip argument).  layout: the leaves of cmcd_layout, gamma included; use_net = 0
 * reads vd, eps, gamma and mgridref_y only.  The leaf `eta` of the reference's tree is not read by this mode (gradient 0).
 * out_loss / out_z / out_stats as cmcd_bound_forward.  grad (nullable: forward only) [n_params], overwritten: omega * sum_n
 * d loss_n / d {vd.mean, vd.logdiag, eps, gamma, mgridref_y, sn}, zeros elsewhere; omega = 1 / N_total.  The positions and
 * momenta do not depend on the network, so d / d sn is local per (particle, bridge) with the cotangent
 * -omega (rho - m_b) on s; only vd, eps, gamma and mgridref_y take a reverse sweep, which is network-free.  The forward call
 * and the gradient call return the same loss bits, repeated calls the same gradient bits (per-item and per-tile slots summed
 * in a fixed order, no floating-point atomics).  A gradient call keeps 4 nbridges + 2 rows of n dim floats in the workspace
 * (z_0..z_K, rho_0..rho_K, rho'_i and rho_i - m_b,i).  Ownership, stream, no-host-sync and capture rules as cmcd_bound_forward.
 * Instances: gmm, many_gmm (dim 2) on geffner widths up to 64 (emb_dim <= 60; README: 20), funnel (dim 10) on widths 65 .. 80
 * (emb_dim 45 .. 60; README: 48); use_net = 0: the same three (target, dim).  lgcp ("lgcp" in the message), dds and every other
 * width: CMCD_ERR_UNSUPPORTED, and 0 from the size query.  nbridges <= 4096, ngrid <= 32. */
int64_t cmcd_ldvi_workspace_bytes(const cmcd_desc* desc, int32_t use_net, int64_t n, int32_t with_grad);
int cmcd_ldvi_bound_grad(const cmcd_desc* desc, const cmcd_layout* layout, int32_t use_net, const int32_t* seeds, int64_t n,
                         const float* params, int64_t n_params, const float* target_consts, int64_t n_target, float omega,
                         void* workspace, int64_t workspace_bytes,
                         float* out_loss, float* out_z, double* out_stats, float* grad /* nullable: forward only */, void* stream);

/* ---- The reverse-time chain of LDVI (use_net = 1: "MCD_U_a-lp-sn", use_net = 0: "MCD_U_a-lp"): cmcd_bound_reverse_uha's chain
 * with three differences — the forward kernel has no network, the step size is the scalar leaf eps (no cos^2 table), grad log p
 * is not clipped.  The Python mirror is cmcd_amd.reverse_ldvi, the float64 restatement tests/reverse_ldvi_restatement.py.  No
 * analogue in the reference; the arithmetic is the forward chain's of cmcd_ldvi_bound_grad walked the other way.  With
 * eta = gamma eps, sigma = sqrt(2 eta), gU(z, b) = -(b grad log p(z) + (1 - b) grad log q(z)) and the betas, the network
 * s([z; rho], i) and q of cmcd_ldvi_bound_grad for the same (desc, layout, params) (the leaf `eta` is not read), particle p runs
 *   z_K = x_p;  rho_K = normal(R);  w = log p(z_K) + log N(rho_K; 0, I)
 *   for i = K-1 .. 0:
 *             rho'' = rho_{i+1} + eps gU(z_{i+1}, beta_i) / 2          (the closing half-kick undone)
 *             z_i   = z_{i+1} - eps rho''                              (the drift undone)
 *             rho'  = rho'' + eps gU(z_i, beta_i) / 2                  (the opening half-kick undone)
 *             m_b   = rho' (1 - eta) [+ 2 eta s([z_i; rho'], i)]       (the network only with use_net = 1; index i)
 *             rho_i = m_b + sigma xi_r,  r = K-1-i
 *             m_f   = rho_i (1 - eta)                                  (no network in the forward kernel)
 *             w    += log N(rho_i; m_b, sigma) - log N(rho'; m_f, sigma)
 *   w -= log q(z_0) + log N(rho_0; 0, I)
 * so w is the functional cmcd_ldvi_bound_grad returns as -loss, on a path drawn from p(z_K) N(rho_K) prod B_i: E[w] >= ln Z.
 * Key chain: cmcd_bound_reverse_uha's (the forward chain's without its first draw).  One rotated loop m = K .. 0 with a single
 * target-evaluation site: K + 1 target evaluations and K network evaluations.
 *   x[n*dim], seeds[n] [device]  ->  out_w[n], out_z0[n*dim], out_rho0[n*dim] [device, float32], out_stats[5] [device, float64]
 *   over l := w, as cmcd_bound_reverse_uha.  A particle whose x row holds a non-finite entry, whose log p(x) is under many_gmm's
 *   floor, or whose w comes out NaN gets w = +inf (weight 0); the other particles of its tile keep their bits.
 * desc and layout as cmcd_ldvi_bound_grad reads them.  Workspace of cmcd_reverse_ldvi_workspace_bytes (the forward part of
 * cmcd_ldvi_workspace_bytes; 0 where the call is unsupported).  Every call runs the prep launch.  No float atomics, repeated
 * calls return equal bits; no host read-back, capturable.  Instances exactly cmcd_ldvi_bound_grad's eight (gmm / many_gmm on 2
 * and 4 neuron tiles, funnel dim 10 on 5, the three network-free ones); lgcp, dds and other widths: CMCD_ERR_UNSUPPORTED.
 * Null pointer, n < 1: CMCD_ERR_BAD_ARG; a short or misaligned workspace: CMCD_ERR_WORKSPACE. */
int64_t cmcd_reverse_ldvi_workspace_bytes(const cmcd_desc* desc, int32_t use_net, int64_t n);
int cmcd_bound_reverse_ldvi(const cmcd_desc* desc, const cmcd_layout* layout, int32_t use_net,
                            const int32_t* seeds, const float* x, int64_t n,
                            const float* params, int64_t n_params,
                            const float* target_consts, int64_t n_target,
                            void* workspace, int64_t workspace_bytes,
                            float* out_w /*[n]*/, float* out_z0 /*[n*dim]*/, float* out_rho0 /*[n*dim]*/,
                            double* out_stats /*[5]*/, void* stream);

/* ---- The reverse-time chain of UHA (Hamiltonian AIS, cmcd_hais_bound_grad): the forward leap-frogs run backwards; the
 * momentum refresh rho = eta rho_prev + sqrt(1 - eta^2) s xi is reversible with respect to N(0, s^2), so its backward kernel is
 * the refresh itself.  The Python mirror is cmcd_amd.reverse_hais, the float64 restatement tests/reverse_hais_restatement.py.
 * With s = exp(md), L = lfsteps, gU and the betas of cmcd_hais_bound_grad, particle p runs
 *   z_K = x_p;  r = s normal(R);  w = log p(z_K)
 *   for i = K-1 .. 0:
 *     w  += log N(r; 0, s)
 *     rho = r + eps gU(z, beta_i) / 2
 *     (L - 1) times:  z -= eps rho / s^2;  rho += eps gU(z, beta_i)
 *     z  -= eps rho / s^2;  rho += eps gU(z, beta_i) / 2              (now (z_i, rho_i))
 *     w  -= log N(rho; 0, s)
 *     r   = eta rho + sqrt(1 - eta^2) s xi_r,  r = K-1-i             (the refresh, reversed)
 *   w -= log q(z_0)
 * i.e. the functional cmcd_hais_bound_grad returns as -loss on a path drawn from p(z_K) N(r; 0, s) prod (reversed steps).  The
 * two densities of a bridge share their constant: w takes sum_j (rho_j^2 - r_j^2) / (2 s_j^2).  K L + 1 target evaluations: the
 * one that ends a bridge's leap-frog opens the next one's.  Key chain and the +inf conventions as cmcd_bound_reverse_ldvi.
 * out_rho0 receives the last r (the chain's initial momentum).  Targets gmm, many_gmm (dim 2), funnel (dim 10); lgcp (no exact
 * draws, "lgcp" in the message) and every other (target, dim): CMCD_ERR_UNSUPPORTED, 0 from the size query.  nbridges, lfsteps
 * < 1: CMCD_ERR_BAD_ARG; nbridges > 4096 or nbridges * lfsteps > 2^24: CMCD_ERR_UNSUPPORTED.  The workspace holds one statistics
 * record per 16-particle tile.  One launch plus the merge; no float atomics, no host read-back, capturable. */
int64_t cmcd_reverse_hais_workspace_bytes(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, int64_t n);
int cmcd_bound_reverse_hais(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout* layout,
                            const int32_t* seeds, const float* x, int64_t n,
                            const float* params, int64_t n_params,
                            const float* target_consts, int64_t n_target,
                            void* workspace, int64_t workspace_bytes,
                            float* out_w /*[n]*/, float* out_z0 /*[n*dim]*/, float* out_rho0 /*[n*dim]*/,
                            double* out_stats /*[5]*/, void* stream);

/* ---- Resumable segments of the LDVI forward chain (use_net = 1: "MCD_U_a-lp-sn", use_net = 0: "MCD_U_a-lp"):
 * cmcd_bound_segment_uha for the first momentum baseline — bridges [k0, k1) from (z, rho, wpath, key).  The Python driver is
 * cmcd_amd.smc_ldvi, the float64 restatement tests/smc_ldvi_restatement.py.  No analogue in the reference; the arithmetic is
 * cmcd_ldvi_bound_grad's bridge, unchanged, cut at a bridge.  With eta = gamma eps, sigma = sqrt(2 eta),
 * gU(z, b) = -(b grad log p(z) + (1 - b) grad log q(z)) (no clip) and the betas, the network s([z; rho], i) and q of
 * cmcd_ldvi_bound_grad for the same (desc, layout, params) (the leaf `eta` is not read), particle p runs
 *   k0 == 0:  key chain, z_0 and rho_0 of cmcd_ldvi_bound_grad (= cmcd_bound_segment_uha's);
 *             wpath = -log q(z_0) - log N(rho_0; 0, I);  gen = gen_0
 *   k0  > 0:  z = z_inout[p], rho = rho_inout[p], wpath = wpath_inout[p], gen = key_inout[p]   (the forward chain's gen_k0)
 *   for i = k0 .. k1-1, the forward call's bridge i:
 *             m_f = rho (1 - eta)                                       (no network in the forward kernel)
 *             rho' = m_f + sigma xi_i,  xi_i = normal(first(split(gen)))
 *             rho'' = rho' - eps gU(z, beta_i) / 2;  z' = z + eps rho'';  rho_new = rho'' - eps gU(z', beta_i) / 2
 *             m_b = rho' (1 - eta) [+ 2 eta s([z; rho'], i)]            (the old z; the network only with use_net = 1)
 *             wpath += log N(rho; m_b, sigma) - log N(rho'; m_f, sigma);   (z, rho) <- (z', rho_new);
 *             gen <- second(split(second(split(gen))))
 *   lg = log gamma_k1(z) + log N(rho; 0, I):  gamma_K = p;  0 < k < K:  log gamma_k = beta_{k-1} log p + (1 - beta_{k-1}) log q
 *   out:  z_inout[p] = z, rho_inout[p] = rho, wpath_inout[p] = wpath, key_inout[p] = gen_k1, out_lg[p] = lg;
 *         out_stats[5] = the statistics of cmcd_bound_forward over l := -(wpath + lg).
 * log p = -inf (the many_gmm floor) gives lg = -inf, never 0 * inf; a NaN stays NaN.  At k1 == nbridges, -(wpath + lg) is the loss
 * of cmcd_ldvi_bound_grad.  The momentum's density is part of lg for the reason given at cmcd_bound_segment_uha (the leap-frog is
 * a volume-preserving bijection of (z, rho), so exp(wpath + lg) is a proper weight for gamma_k1(z) N(rho; 0, I)); a resampling
 * stage restarts its offspring with wpath = -lg[ancestor], moves z AND rho with the same ancestors and leaves key_inout alone.
 * ONE runtime-bounded rotated loop m = k0 .. k1 with a single site that evaluates (log p, grad log p, grad log q) at z_m (it
 * closes bridge m - 1, opens bridge m, forms lg at m == k1); the network evaluation of a bridge stays inside the bridge, at one
 * site.  So [0, k) then [k, K) returns the BITS of [0, K) in z, rho, wpath, lg and the key, at one extra target evaluation per cut.
 *   0 <= k0 < k1 <= nbridges, else CMCD_ERR_BAD_ARG;  seeds[n] is read when k0 == 0 (null there: CMCD_ERR_BAD_ARG) and may be
 *   null otherwise.  Buffers as cmcd_bound_segment_uha.  A short or misaligned workspace: CMCD_ERR_WORKSPACE.
 * desc and layout as cmcd_ldvi_bound_grad reads them.  Workspace of cmcd_segment_ldvi_workspace_bytes (the forward part of
 * cmcd_ldvi_workspace_bytes; 0 where the call is unsupported).  Every call runs the prep launch.  Every refusal is made on the
 * host before anything touches the device; no float atomics, repeated calls return equal bits; no host read-back, capturable.
 * Instances exactly cmcd_ldvi_bound_grad's eight (gmm / many_gmm on 2 and 4 neuron tiles, funnel dim 10 on 5, the three
 * network-free ones); lgcp ("lgcp" in the message), dds and other widths: CMCD_ERR_UNSUPPORTED.  No cooperative form. */
int64_t cmcd_segment_ldvi_workspace_bytes(const cmcd_desc* desc, int32_t use_net, int64_t n);
int cmcd_bound_segment_ldvi(const cmcd_desc* desc, const cmcd_layout* layout, int32_t use_net, int32_t k0, int32_t k1,
                            const int32_t* seeds /* k0 == 0; else nullable */, int64_t n,
                            const float* params, int64_t n_params,
                            const float* target_consts, int64_t n_target,
                            void* workspace, int64_t workspace_bytes,
                            float* z_inout /*[n*dim]*/, float* rho_inout /*[n*dim]*/, float* wpath_inout /*[n]*/,
                            uint32_t* key_inout /*[n*2]*/, float* out_lg /*[n]*/, double* out_stats /*[5]*/, void* stream);

/* ---- Resumable segments of the UHA forward chain (Hamiltonian AIS, cmcd_hais_bound_grad): bridges [k0, k1) from
 * (z, rho, wpath, key), where rho is the momentum BETWEEN bridges — rho_prev of the write-out at cmcd_hais_bound_grad, the
 * momentum that left bridge k0 - 1 (s normal(R) at k0 == 0).  The Python driver is cmcd_amd.smc_hais, the float64 restatement
 * tests/smc_hais_restatement.py.  With s = exp(md), L = lfsteps, gU and the betas of cmcd_hais_bound_grad, particle p runs
 *   k0 == 0:  key chain, z_0 and rho_prev = s normal(R) of cmcd_hais_bound_grad;  wpath = -log q(z_0);  gen = gen_0
 *   k0  > 0:  z = z_inout[p], rho_prev = rho_inout[p], wpath = wpath_inout[p], gen = key_inout[p]
 *   for i = k0 .. k1-1, the forward call's bridge i:
 *             rho = eta rho_prev + sqrt(1 - eta^2) s xi_i                                       (the refresh)
 *             r = rho - eps/2 gU(z, beta_i);  z += eps r / s^2;  (L - 1) times:  r -= eps gU(z, beta_i);  z += eps r / s^2
 *             r -= eps/2 gU(z, beta_i)                                                          (the L-step leap-frog)
 *             wpath += log N(r; 0, s) - log N(rho; 0, s);  rho_prev = r;  gen <- second(split(second(split(gen))))
 *   lg = log gamma_k1(z) alone, no momentum term:  gamma_K = p;  0 < k < K:  log gamma_k = beta_{k-1} log p + (1 - beta_{k-1}) log q
 *   out:  z_inout[p] = z, rho_inout[p] = rho_prev, wpath_inout[p] = wpath, key_inout[p] = gen_k1, out_lg[p] = lg;
 *         out_stats[5] over l := -(wpath + lg).  At k1 == nbridges, -(wpath + lg) is the loss of cmcd_hais_bound_grad.
 * Why lg carries no momentum density.  Write M(rho | rho_prev) for the refresh and T_i for the leap-frog of bridge i, a
 * volume-preserving bijection of (z, rho).  The forward path has density  q(z_0) N(rho_prev,0; 0, s) prod_i M(rho_i | r_{i-1})
 * (r_{-1} = rho_prev,0, r_i = what T_i leaves), the backward path started at gamma_k(z_k) N(r_{k-1}; 0, s) and run through the
 * inverted leap-frogs and the refresh  gamma_k(z_k) N(r_{k-1}; 0, s) prod_i M(r_{i-1} | rho_i).  The refresh is reversible with
 * respect to N(0, s^2):  M(rho | r) N(r; 0, s) = M(r | rho) N(rho; 0, s),  so  M(r_{i-1} | rho_i) / M(rho_i | r_{i-1}) =
 * N(r_{i-1}; 0, s) / N(rho_i; 0, s)  and the ratio of the two path densities is
 *     gamma_k(z_k) / q(z_0)  *  N(r_{k-1}) / N(r_{-1})  *  prod_{i<k} N(r_{i-1}) / N(rho_i)
 *   = gamma_k(z_k) / q(z_0)  *  prod_{i<k} N(r_i; 0, s) / N(rho_i; 0, s):
 * the momentum densities telescope, the functional has neither an initial nor a final momentum term (as the forward call's has
 * none), and what is left is exp(wpath + lg) with lg = log gamma_k(z) alone — a proper weight for gamma_k(z) N(rho_prev; 0, s^2)
 * on the PAIR (z, rho_prev).  That is why the overdamped restart rule wpath_j = -lg[a_j] is still right here (the offspring
 * of a resampling stage are equally weighted draws of that joint law: wpath + lg = 0), and why a stage must move rho with z:
 * the law that is resampled is the joint one, and a z with another particle's momentum is not a draw of it.  Keys stay with
 * their slot.
 * The kernel is ONE runtime loop over the evaluations m = k0 L .. k1 L with a single site that evaluates (log p, grad log p,
 * grad log q): the evaluation that closes one bridge opens the next and forms lg at m = k1 L — (k1 - k0) L + 1 target
 * evaluations per segment, so a cut costs one extra.  [0, k) then [k, K) returns the BITS of [0, K) in z, rho, wpath, lg and
 * the key.
 *   0 <= k0 < k1 <= nbridges, else CMCD_ERR_BAD_ARG;  seeds[n] is read when k0 == 0 (null there: CMCD_ERR_BAD_ARG).  Buffers as
 *   cmcd_bound_segment_uha; a short or misaligned workspace: CMCD_ERR_WORKSPACE.
 * Targets gmm, many_gmm (dim 2), funnel (dim 10); lgcp ("lgcp" in the message: cmcd_hais_lgcp_bound_grad runs whole chains
 * only) and every other (target, dim): CMCD_ERR_UNSUPPORTED, 0 from the size query.  nbridges, lfsteps < 1: CMCD_ERR_BAD_ARG;
 * nbridges > 4096 or nbridges * lfsteps > 2^24: CMCD_ERR_UNSUPPORTED (the forward call's limits).  The workspace holds one
 * statistics record per 16-particle tile.  One launch plus the merge; every refusal on the host before anything touches the
 * device; no float atomics, repeated calls return equal bits; no host read-back, capturable. */
int64_t cmcd_segment_hais_workspace_bytes(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, int64_t n);
int cmcd_bound_segment_hais(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout* layout,
                            int32_t k0, int32_t k1, const int32_t* seeds /* k0 == 0; else nullable */, int64_t n,
                            const float* params, int64_t n_params,
                            const float* target_consts, int64_t n_target,
                            void* workspace, int64_t workspace_bytes,
                            float* z_inout /*[n*dim]*/, float* rho_inout /*[n*dim]*/, float* wpath_inout /*[n]*/,
                            uint32_t* key_inout /*[n*2]*/, float* out_lg /*[n]*/, double* out_stats /*[5]*/, void* stream);

/* ---- Optimiser step of the training loop (/root/reference/src/opt.py:14-35,100-116) fused into one launch:
 * g = clip(grad, +-clip); Adam moments (optax.adam: bias correction 1 - b^step, eps outside the root);
 * params += -lr * m_hat / (sqrt(v_hat) + eps); projection of the listed ranges (opt.py:14-24);
 * optional ema = (1 - ema_step) ema + ema_step params (optax.incremental_update, opt.py:114-116).
 * step is the 1-based iteration count.  All pointers device, length n; ema may be NULL.
 * Non-finite input follows the reference: optax.clip passes a NaN gradient through (the parameter becomes NaN and the
 * next loss trips the check), +-inf is clipped.  Divergence guard (opt.py:122-124 `if isnan(mean(loss)): return` BEFORE
 * the update): with `losses` [n_losses] (device, nullable) the launch first decides whether mean(losses) is NaN — some
 * loss is NaN, or +inf and -inf both occur — and if so leaves params / moments / ema untouched and sets *diverged = 1
 * (device int32, sticky, nullable; once set every later guarded step is skipped too), so the caller may poll the flag
 * at leisure and still gets back the last parameters the reference would have returned. */
enum { CMCD_PROJECT_CLAMP = 0,      /* x -> min(max(x, lo), hi) */
       CMCD_PROJECT_RELU_FLOOR = 1  /* x -> relu(x - lo) + lo   (mgridref_y, opt.py:22-23) */ };
typedef struct cmcd_project_range {
  int64_t offset, length;
  int32_t kind, reserved;
  float lo, hi;
} cmcd_project_range;
int cmcd_adam_step(float* params, const float* grad, float* mu, float* nu, float* ema, int64_t n,
                   float lr, float b1, float b2, float eps, float clip, int64_t step, float ema_step,
                   const cmcd_project_range* ranges, int32_t n_ranges,
                   const float* losses, int64_t n_losses, int32_t* diverged, void* stream);
/* The same step with the iteration count on the device (*step_counter = completed steps, int64, incremented by the
 * call): every launch argument is then constant across iterations, so a whole training iteration (gradient call
 * + this) can be captured once in a hipGraph and replayed (cmcd_amd.opt.run does, for launch-bound configs). */
int cmcd_adam_step_dev(float* params, const float* grad, float* mu, float* nu, float* ema, int64_t n,
                       float lr, float b1, float b2, float eps, float clip, int64_t* step_counter, float ema_step,
                       const cmcd_project_range* ranges, int32_t n_ranges,
                       const float* losses, int64_t n_losses, int32_t* diverged, void* stream);

/* Device-side merge of `count` statistics vectors rows[count][5] (e.g. the result of an RCCL
 * all-gather of every rank's out_stats, in rank order) into out5[5], fixed order, one small kernel
 * on `stream`.  [device] pointers. */
int cmcd_stats_merge_device(const double* rows, int32_t count, double* out5, void* stream);

/* Host-side, no GPU: merge `count` stats vectors (e.g. one per rank, after an all-gather) in
 * the given fixed order, then produce mean, var(ddof=0), lnZ = logsumexp(-l) - log n_total.
 * n_per[i] = number of particles behind stats[i].  out3 = {mean, var, lnZ}. */
int cmcd_stats_merge(const double* stats, const int64_t* n_per, int32_t count,
                     double* merged5, double* out3);

/* ---- Importance diagnostics and systematic resampling of the weighted particle system an entry point returned:
 * loss[n] and z[n, dim] with weights w_j = exp(-loss_j).  No analogue in the reference, which stops at the unweighted z and
 * logsumexp(-loss); the arithmetic is restated in float64 NumPy in tests/test_gpu_resample.py.
 * The n rows are `groups` consecutive groups of m = n / groups rows (the n_input_dist_seeds x n_samples layout of the
 * evaluation); each group is treated on its own, all sums in float64 and in a fixed order (same arguments, same bits):
 *   M = max(-loss) over the finite entries, w_j = exp(-loss_j - M) (a loss of +inf weighs 0), S1 = sum w, S2 = sum w^2
 *   out_stats[g] = {number of finite losses, ln Z = M + log S1 - log m, ESS = S1^2 / S2, max_j w_j / S1, diverged}
 *   a group holding a NaN or -inf loss is diverged: {NaN, NaN, NaN, NaN, 1} and the identity as ancestors;
 *   a group without a finite loss: {0, -inf, 0, 0, 0} and the identity as ancestors.
 * Systematic resampling: u_g = word g of jax.random.uniform(PRNGKey(seed), (groups,)) (Threefry, as everywhere in this
 * library), thresholds t_k = (k + u_g) / m, ancestor a_k = min{ j : C_j > t_k } with C the inclusive cumulative sum of w / S1,
 * never past the last row of positive weight.  out_index[n] (int32, nullable) receives the ancestors as global row numbers,
 * out_z[n, dim] (nullable; needs z, must not overlap it) the rows z[a_k, :].  With both null only out_stats is written.
 * m <= 2^20 (CMCD_ERR_UNSUPPORTED above), n < 2^31.  One launch on `stream`, no host synchronisation, no allocation: it can be
 * captured into a hipGraph behind the forward call that produced loss and z.  All pointers [device]. */
int64_t cmcd_resample_workspace_bytes(int64_t n, int32_t groups);   /* 0 on bad arguments */
int cmcd_resample_systematic(const float* loss, const float* z, int64_t n, int32_t dim, int32_t groups, uint32_t seed,
                             void* workspace, int64_t workspace_bytes, int32_t* out_index, float* out_z,
                             double* out_stats /*[groups][5]*/, void* stream);

/* ---- Batched entropic optimal transport between equal-size point clouds: the evaluation's Sinkhorn W2
 * (/root/reference/src/utils.py:207-216, `ot.sinkhorn2(a, b, M / M.max(), reg)`), float64 throughout, `groups` independent
 * problems per call.  Problem g has clouds x[g][n][dim], y[g][n][dim] and weights a[g][n], b[g][n] (a null pointer = uniform
 * 1 / n):  M_ij = ||x_i - y_j||^2 / max_ij ||x_i - y_j||^2,  K = exp(-M / reg),  u = v = 1 / n;  iteration `it` = 0, 1, ...:
 * v <- b / (K^T u), u <- a / (K v), and when it % 10 == 0: err = sum_j (v_j (K^T u)_j - b_j)^2, stop if err < stop_thr; at most
 * num_iter_max iterations;  cost = sum_ij u_i K_ij v_j M_ij.  The arithmetic is restated in tests/test_gpu_sinkhorn.py.
 * Three calls share one workspace, whose content is the state of the solve:
 *   setup    builds K, the initial u and K^T u.  A problem with a non-finite coordinate or weight, or whose points all
 *            coincide (max M = 0), is finished at once with status 2.
 *   iterate  enqueues the iterations first_iteration ... first_iteration + count - 1, one launch each (and, when that reaches
 *            num_iter_max, one more launch that takes the last check and closes the problems at the cap).  Successive calls
 *            must continue where the previous one stopped.  A finished problem costs its workgroups one load.
 *            done_flags[groups] (int32, nullable) receives 1 for every finished problem.
 *   cost     writes out[g] = {cost, iterations carried out, err at the last check (NaN before the first), status} as four
 *            doubles; status 0 converged, 1 cap reached (or not finished yet), 2 not solvable (cost NaN).
 * Every sum is taken in an order fixed by n alone (row tiles of 64, workgroups of 256): a problem's bits do not depend on
 * the other problems of the call, on which of them are finished, or on the stream.  No floating-point atomics.
 * 2 <= n <= 8192 and groups <= 65535 (CMCD_ERR_UNSUPPORTED above), dim >= 1.  Workspace, with T = ceil(n / 64):
 *   bytes = 32 groups + 8 (groups n^2 + 5 groups n + 2 groups T n + groups T), rounded up to a multiple of 16.
 * No call synchronises or allocates; all three can be captured into a hipGraph.  All pointers [device]. */
int64_t cmcd_sinkhorn_workspace_bytes(int64_t n, int32_t dim, int32_t groups);   /* 0 on bad arguments */
int cmcd_sinkhorn_setup(const double* x, const double* y, const double* a /*nullable*/, const double* b /*nullable*/, int64_t n,
                        int32_t dim, int32_t groups, double reg, void* workspace, int64_t workspace_bytes, void* stream);
int cmcd_sinkhorn_iterate(int64_t n, int32_t dim, int32_t groups, int32_t first_iteration, int32_t count,
                          int32_t num_iter_max, double stop_thr, void* workspace, int64_t workspace_bytes,
                          int32_t* done_flags /*[groups], nullable*/, void* stream);
int cmcd_sinkhorn_cost(const double* x, const double* y, int64_t n, int32_t dim, int32_t groups, void* workspace,
                       int64_t workspace_bytes, double* out /*[groups][4]*/, int32_t* done_flags /*[groups], nullable*/,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CMCD_HIP_H */
