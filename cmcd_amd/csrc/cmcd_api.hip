// libcmcd_hip.so — the C ABI of include/cmcd_hip.h and the hooks of include/cmcd_hip_diag.h.  Host code only: every kernel is
// launched through its own file's launcher (cmcd_host.h for cmcd_kernels.hip, cmcd_common.h for the others).
//
// One call = validate -> plan (CallPlan: effective descriptor + workspace carve-up) -> prep tables -> choose and launch the
// trajectory kernel -> merge the statistics (-> reverse sweep, for the gradient entry points).  All on the caller's stream,
// no host sync.  The size queries are the same plan, built for the largest target-constant block.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "cmcd_common.h"
#include "cmcd_hip.h"
#include "cmcd_hip_diag.h"
#include "cmcd_host.h"

namespace cmcd {

static thread_local char g_err[512] = "";
static thread_local char g_kernel_name[96] = "";   // cmcd_last_kernel_name

// Optional in-library timing of the trajectory kernel: when enabled, every cmcd_bound_forward
// brackets its traj_kernel launch with a hipEvent pair on the caller's stream (bench.py reads
// the average kernel duration from them for the roofline figure).
struct ProfileState {
  static constexpr int kMax = 4096;
  bool on = false;
  bool open = false;   // profile_begin recorded the start event of pair `used`
  int used = 0;
  hipEvent_t ev[kMax][2];
  int created = 0;
};
static thread_local ProfileState g_prof;
// cmcd_debug_capture_noise: armed per host thread, consumed (and cleared) by the next forward call on that thread
struct NoiseCapture { uint32_t* bits = nullptr; uint32_t* keys = nullptr; float* noise = nullptr; };
static thread_local NoiseCapture g_capture;

int fail(int code, const char* fmt, const char* a, long long b) {
  snprintf(g_err, sizeof(g_err), fmt, a, b);
  return code;
}
int fail_msg(int code, const char* msg) { return fail(code, "%s", msg); }

// the profile's event pair around the trajectory launch (when cmcd_profile_enable is on): profile_begin right in front of the
// launch, profile_end behind it; a launch that fails in between leaves no record
static int profile_begin(hipStream_t stream) {
  g_prof.open = g_prof.on && g_prof.used < ProfileState::kMax;
  if (!g_prof.open) return CMCD_OK;
  if (g_prof.used >= g_prof.created) {
    CMCD_HIP_CHECK(hipEventCreate(&g_prof.ev[g_prof.created][0]));
    CMCD_HIP_CHECK(hipEventCreate(&g_prof.ev[g_prof.created][1]));
    ++g_prof.created;
  }
  CMCD_HIP_CHECK(hipEventRecord(g_prof.ev[g_prof.used][0], stream));
  return CMCD_OK;
}
static int profile_end(hipStream_t stream) {
  if (!g_prof.open) return CMCD_OK;
  g_prof.open = false;
  CMCD_HIP_CHECK(hipEventRecord(g_prof.ev[g_prof.used][1], stream));
  ++g_prof.used;
  return CMCD_OK;
}
// traj_launch calls this once its checks have passed, right in front of the kernel launch
static int traj_before_launch(hipStream_t stream) {
  const int rc = profile_begin(stream);
  if (rc == CMCD_OK) snprintf(g_kernel_name, sizeof(g_kernel_name), "traj_kernel");
  return rc;
}

// Tiles (16 particles each) up to which the CU-cooperative kernel is preferred; measured crossovers on
// MI355X (tools/probes/variant_sweep.py, t9_variants.py): dds/geffner T<=4 between 512 and 1024 tiles; the 132-wide
// net at ~600 (500 tiles: cooperative 1.85 ms against 2.27 ms one wave per tile; 1000 tiles: 3.69 against 2.28).
// r02, after the cooperative kernel's per-bridge time dropped by a sixth (tools/probes/variant_crossover.py,
// profiles/r02_s2e_variant_crossover.txt; the cooperative time is ceil(tiles / 256 CUs) rounds of one workgroup per CU):
//   dds net, 40-mode mixture:     cooperative wins through 6 rounds (1536 tiles: 1.13 against 1.34 ms; 2048: 1.42 / 1.34)
//   132-wide net, 40-mode mixture: through 3 rounds (768 tiles: 1.91 against 2.31 ms; 813: 2.53 / 2.29)
//   funnel / gmm on the narrow geffner nets: 512 tiles still (768: 0.373 / 0.314 ms and 0.0257 / 0.0246 ms)
static int coop_max_tiles(const cmcd_desc& d, int T) {
  if (d.target == CMCD_TARGET_MANY_GMM && d.dim == 2) {
    if (d.arch == CMCD_ARCH_DDS) return 1536;
    if (T == 9) return 768;
  }
  return 512;
}

static inline int64_t align4(int64_t x) { return (x + 3) & ~int64_t(3); }

static bool hidden_width(const cmcd_desc& d, int& HP) {
  if (d.arch == CMCD_ARCH_DDS) { HP = 64; return true; }
  if (d.arch == CMCD_ARCH_GEFFNER) {
    if (d.emb_dim < 1) return false;
    HP = ((net_in_dim(d) + d.emb_dim + 15) / 16) * 16;
    if (d.mode == CMCD_MODE_CAIS_UHA_SN && d.target != CMCD_TARGET_LGCP) {
      // 2nd-order CMCD has its own kernels (cmcd_uha.hip): instances of 2, 4, 5 and 9 neuron tiles (gmm 2*2+20 = 24,
      // funnel 2*10+48 = 68, the 40-mode mixture 2*2+130 = 134), other widths zero-padded to the next one
      const int T = HP / 16;
      HP = 16 * (T <= 2 ? 2 : (T <= 4 ? 4 : (T <= 5 ? 5 : (T <= 9 ? 9 : T))));
      return true;
    }
    // Kernel instances exist for 2, 4 and 9 neuron tiles (the BASELINE widths 22 / 58 / 132); any other width runs
    // on the next larger instance with zero-padded weights: a padded unit has no outgoing weight, so it cannot
    // reach the output, and its gradient entries are never copied out.  (lgcp has its own path: any width.)
    if (d.target != CMCD_TARGET_LGCP) {
      const int T = HP / 16;
      // funnel (d = 10): its gradient kernels start at 4 tiles, and forward / gradient share one workspace layout
      const int tmin = d.target == CMCD_TARGET_FUNNEL ? 4 : 2;
      HP = 16 * (T <= tmin ? tmin : (T <= 4 ? 4 : (T <= 9 ? 9 : T)));
    }
    return true;
  }
  return false;
}

// width of the state part of the network input: z, or concat(z, rho) for the momentum mode (rho_dim = dim,
// the reference's src/mcdboundingmachine.py:82-98)
int net_in_dim(const cmcd_desc& d) { return d.mode == CMCD_MODE_CAIS_UHA_SN ? 2 * d.dim : d.dim; }

// floats of the trajectory a gradient call keeps: z_0..z_K, plus rho_0..rho_K and rho'_0..rho'_{K-1} for the momentum mode
static int64_t kept_traj_floats(const cmcd_desc& d, int64_t n) {
  return (int64_t)(d.mode == CMCD_MODE_CAIS_UHA_SN ? 3 * d.nbridges + 2 : d.nbridges + 1) * n * d.dim;
}

// the schedule tables every layout starts with -> their floats
static int64_t sched_tables(int64_t K, WsLayout& w) {
  int64_t o = 0;
  w.beta = o; o += align4(K);
  w.eps = o; o += align4(K);
  w.sig = o; o += align4(K);
  w.logsig = o; o += align4(K);
  w.sched = o; o += 8 * K;
  return o;
}

// lgcp: only the schedule tables live in the common layout; the rest is carved by cmcd_lgcp.hip
static void make_ws_lgcp(const cmcd_desc& d, int64_t n, WsLayout& w) {
  memset(&w, 0, sizeof(w));
  w.total_floats = sched_tables(d.nbridges, w);
  w.n_waves = (int32_t)n;  // one statistics record per particle
}

static bool make_ws(const cmcd_desc& d, int64_t n, int64_t n_target, WsLayout& w) {
  int HP;
  if (!hidden_width(d, HP)) return false;
  const int64_t K = d.nbridges, D = d.dim;
  w.HP = HP;
  w.T = HP / 16;
  int64_t o = sched_tables(K, w);
  w.bias1 = o; o += (K + 1) * HP;
  if (d.arch == CMCD_ARCH_GEFFNER) { w.utab = o; o += (K + 1) * HP; } else { w.utab = w.bias1; }
  w.w1z = o; o += int64_t(net_in_dim(d)) * HP;
  w.w2 = o; o += int64_t(HP) * HP;
  w.w2t = o; o += int64_t(HP) * HP;
  w.w2q = o; o += 2 * int64_t(HP) * HP;
  w.b2 = o; o += HP;
  w.w3t = o; o += D * HP;
  w.b3 = o; o += 16;
  w.tgt_floats = d.target == CMCD_TARGET_MANY_GMM ? align4(4 + (n_target - 1)) : 0;   // staged for LDS: header + means
  w.tgt = o; o += w.tgt_floats;
  o = (o + 1) & ~int64_t(1);
  w.n_waves = int32_t((n + 15) / 16);
  // sized for the cooperative kernel's 8-particle tiles (twice the records of the 16-particle tiling)
  w.partials = o; o += int64_t((n + 7) / 8) * CMCD_NSTATS * 2;
  w.total_floats = o;
  return true;
}

// What a set of prepared tables was formed from, as far as the library can know it without reading device memory: FNV-1a
// over the descriptor (minus the kernel-variant field, which selects a kernel and not a table), the layout and the sizes.
// The caller's descriptor, not the plan's effective one.
static uint32_t tables_stamp(const cmcd_desc& d, const cmcd_layout& lay, int64_t n, int64_t n_params, int64_t n_target) {
  uint32_t h = 2166136261u;
  auto eat = [&](const void* p, size_t len) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < len; ++i) { h ^= b[i]; h *= 16777619u; }
  };
  cmcd_desc dd = d;
  dd.reserved = 0;
  eat(&dd, sizeof dd); eat(&lay, sizeof lay); eat(&n, sizeof n); eat(&n_params, sizeof n_params); eat(&n_target, sizeof n_target);
  return h ? h : 1u;
}

static int check_desc(const cmcd_desc* d) {
  if (!d) return fail(CMCD_ERR_BAD_ARG, "null desc%s");
  if (d->mode < CMCD_MODE_CAIS_SN || d->mode > CMCD_MODE_CAIS_UHA_SN)
    return fail(CMCD_ERR_UNSUPPORTED, "Mode not implemented.%s");
  if (d->mode == CMCD_MODE_ULA && d->arch != CMCD_ARCH_DDS)
    return fail(CMCD_ERR_BAD_ARG, "MCD_ULA has no network: pass arch = CMCD_ARCH_DDS as the placeholder%s");
  if (d->arch != CMCD_ARCH_DDS && d->arch != CMCD_ARCH_GEFFNER)
    return fail(CMCD_ERR_UNSUPPORTED, "nn_arch not implemented%s");
  if (d->nbridges < 1) return fail(CMCD_ERR_BAD_ARG, "nbridges must be >= 1%s");
  if (d->ngrid < 1 || d->ngrid > 32) return fail(CMCD_ERR_BAD_ARG, "ngrid must be in [1, 32]%s");
  if (d->eps_schedule == CMCD_EPS_LINEAR && d->nbridges < 2)
    return fail(CMCD_ERR_BAD_ARG, "linear eps schedule needs nbridges >= 2%s");
  int HP;
  if (!hidden_width(*d, HP)) return fail(CMCD_ERR_BAD_ARG, "bad emb_dim%s");
  if (d->target == CMCD_TARGET_LGCP) {
    if ((d->arch != CMCD_ARCH_GEFFNER && d->mode != CMCD_MODE_ULA) || d->dim < 4 || d->dim > 4096)
      return fail(CMCD_ERR_UNSUPPORTED, "lgcp runs with the geffner net only%s");
    return CMCD_OK;
  }
  if (d->mode == CMCD_MODE_CAIS_UHA_SN) {
    if (!uha_available(*d, HP / 16))
      return fail(CMCD_ERR_UNSUPPORTED, "no MCD_CAIS_UHA_sn kernel instance for this (target, dim, arch, width=%s%lld)", "", HP);
    return CMCD_OK;
  }
  if (!traj_available(*d, HP / 16))
    return fail(CMCD_ERR_UNSUPPORTED, "no kernel instance for this (target, dim, arch, width=%s%lld)", "", HP);
  return CMCD_OK;
}

static int check_workspace(const void* ptr, int64_t bytes, int64_t need) {
  if (bytes < need || (reinterpret_cast<uintptr_t>(ptr) & 15))
    return fail(CMCD_ERR_WORKSPACE, "workspace too small or not 16-byte aligned (need %s%lld bytes)", "", need);
  return CMCD_OK;
}

// every leaf this configuration reads must lie inside params_flat
static bool layout_inside(const cmcd_desc& d, const cmcd_layout& lay, int64_t n_params) {
  const int64_t K = d.nbridges, D = d.dim, E = d.emb_dim, DIN = net_in_dim(d), IN = DIN + E;
  auto need = [&](int64_t off, int64_t len) { return off >= 0 && off + len <= n_params; };
  bool ok = need(lay.vd_mean, D) && need(lay.vd_logdiag, D) && need(lay.eps, 1) && need(lay.mgridref_y, d.ngrid + 1) &&
            (d.mode != CMCD_MODE_CAIS_UHA_SN || need(lay.gamma, 1));
  if (d.mode == CMCD_MODE_ULA) {
    // no network leaves
  } else if (d.arch == CMCD_ARCH_GEFFNER)
    ok = ok && need(lay.g_emb, K * E) && need(lay.g_factor, 1) && need(lay.g_w1, IN * IN) && need(lay.g_b1, IN) &&
         need(lay.g_w2, IN * IN) && need(lay.g_b2, IN) && need(lay.g_w3, IN * D) && need(lay.g_b3, D);
  else
    ok = ok && need(lay.d_phase, 64) && need(lay.d_tw1, 128 * 64) && need(lay.d_tb1, 64) && need(lay.d_tw2, 64 * 64) &&
         need(lay.d_tb2, 64) && need(lay.d_sw1, (DIN + 64) * 64) && need(lay.d_sb1, 64) && need(lay.d_sw2, 64 * 64) &&
         need(lay.d_sb2, 64) && need(lay.d_sw3, 64 * D) && need(lay.d_sb3, D);
  return ok;
}

// ------------------------------------------------------------------------------------------
// the plan of one call: what runs (effective descriptor) and where it lives in the caller's workspace
//   forward:     [forward tables + statistics records]
//   reverse:     the forward layout (same tables, one statistics record per 16-particle tile); overdamped modes, no lgcp
//   segment:     the forward layout again (bridges [k0, k1) from a caller-supplied state); overdamped modes, no lgcp
//   segment-uha: the same for MCD_CAIS_UHA_sn (the state carries the momentum); that mode only, no lgcp
//   reverse-uha: the forward layout once more (the reverse-time chain of MCD_CAIS_UHA_sn); that mode only, no lgcp
//   reverse-ldvi: the forward layout of LDVI's effective descriptor (cmcd_ldvi_bound_grad's), no gradient part; no lgcp
//   reverse-hais: [one statistics record per 16-particle tile] (hais_chain_plan below: UHA has no tables and no descriptor)
//   segment-ldvi, segment-hais: the layouts of reverse-ldvi and reverse-hais (bridges [k0, k1) from a state with momentum)
//   var-grad:    [forward | gradient workspace | z_0..z_K | loss, z, statistics of the internal forward]   (the last two: work items only)
//   bound-grad:  [forward | gradient workspace | kept trajectory | work-item scratch]
// ------------------------------------------------------------------------------------------
enum PlanKind { PLAN_FORWARD, PLAN_VAR_GRAD, PLAN_BOUND_GRAD, PLAN_REVERSE, PLAN_SEGMENT, PLAN_SEGMENT_UHA, PLAN_REVERSE_UHA,
                PLAN_REVERSE_LDVI, PLAN_SEGMENT_LDVI };

struct CallPlan {
  cmcd_desc d;      // effective descriptor: the caller's, with what its mode fixes
  WsLayout w;
  int n_mix;
  bool lgcp;
  bool item;        // gradient on work items (small batches) instead of whole chains
  bool keep;        // the forward pass leaves its trajectory at `traj`
  int64_t fwd;      // floats of the forward part (what a forward-only call demands)
  int64_t gfl, traj, scratch;   // float offsets of the gradient workspace, the kept trajectory and the work-item scratch
  int64_t total;    // bytes of this layout = what the size query of `kind` answers
  int64_t need;     // bytes the entry point demands: total, except that the VarGrad calls demand their size query's answer
};

// query: the plan of a size query — n_target is not read, the target block is the largest the target can stage (64 mixtures)
static int make_plan(const cmcd_desc& desc, int64_t n, int64_t n_target, PlanKind kind, bool query, CallPlan& p) {
  cmcd_desc& d = p.d = desc;
  // the overdamped baselines: constant eps, no clipping (the reference's dispatcher passes neither, mcd_utils.py:35-58)
  if (d.mode == CMCD_MODE_ULA || d.mode == CMCD_MODE_ULA_SN) { d.eps_schedule = CMCD_EPS_CONST; d.grad_clipping = 0; }
  // MCD_CAIS_UHA_sn: the cos^2 schedule and the clip are fixed by the function body (mcd_under_lp_a_cais.py:23-48)
  if (d.mode == CMCD_MODE_CAIS_UHA_SN) { d.eps_schedule = CMCD_EPS_COS_SQ; d.grad_clipping = 1; }
  const bool many = d.target == CMCD_TARGET_MANY_GMM;
  if (query) n_target = many ? 1 + 2 * 64 : 0;
  p.n_mix = many ? int((n_target - 1) / 2) : 0;
  p.lgcp = d.target == CMCD_TARGET_LGCP;
  p.item = p.keep = false, p.gfl = p.traj = p.scratch = 0;
  if (p.lgcp) {
    make_ws_lgcp(d, n, p.w);
    p.fwd = lgcp_workspace_floats(d, n, p.w.total_floats);
  } else {
    if (!make_ws(d, n, n_target, p.w)) return fail(CMCD_ERR_BAD_ARG, "bad descriptor%s");
    p.fwd = p.w.total_floats;
  }
  p.total = p.need = p.fwd * 4;
  if (kind == PLAN_FORWARD) return CMCD_OK;
  if (kind == PLAN_REVERSE) {
    if (d.mode == CMCD_MODE_CAIS_UHA_SN)
      return fail(CMCD_ERR_UNSUPPORTED, "the reverse chain exists for the overdamped modes only (MCD_CAIS_UHA_sn has no reverse kernel)%s");
    if (p.lgcp) return fail(CMCD_ERR_UNSUPPORTED, "the reverse chain has no lgcp kernel%s");
    if (!reverse_available(d, p.w.T))
      return fail(CMCD_ERR_UNSUPPORTED, "no reverse-chain kernel instance for this (target, dim, arch, width=%s%lld)", "", p.w.HP);
    return CMCD_OK;
  }
  if (kind == PLAN_SEGMENT) {
    if (d.mode == CMCD_MODE_CAIS_UHA_SN)
      return fail(CMCD_ERR_UNSUPPORTED, "chain segments exist for the overdamped modes only (MCD_CAIS_UHA_sn has no segment kernel)%s");
    if (p.lgcp) return fail(CMCD_ERR_UNSUPPORTED, "chain segments have no lgcp kernel%s");
    if (!segment_available(d, p.w.T))
      return fail(CMCD_ERR_UNSUPPORTED, "no segment kernel instance for this (target, dim, arch, width=%s%lld)", "", p.w.HP);
    return CMCD_OK;
  }
  if (kind == PLAN_SEGMENT_UHA) {
    if (d.mode != CMCD_MODE_CAIS_UHA_SN)
      return fail(CMCD_ERR_UNSUPPORTED, "cmcd_bound_segment_uha is MCD_CAIS_UHA_sn's segment call (the overdamped modes have cmcd_bound_segment)%s");
    if (p.lgcp) return fail(CMCD_ERR_UNSUPPORTED, "chain segments have no lgcp kernel%s");
    if (!segment_uha_available(d, p.w.T))
      return fail(CMCD_ERR_UNSUPPORTED, "no 2nd-order segment kernel instance for this (target, dim, arch, width=%s%lld)", "", p.w.HP);
    return CMCD_OK;
  }
  if (kind == PLAN_REVERSE_UHA) {
    if (d.mode != CMCD_MODE_CAIS_UHA_SN)
      return fail(CMCD_ERR_UNSUPPORTED, "cmcd_bound_reverse_uha is MCD_CAIS_UHA_sn's reverse chain (the overdamped modes have cmcd_bound_reverse)%s");
    if (p.lgcp) return fail(CMCD_ERR_UNSUPPORTED, "the reverse chain has no lgcp kernel%s");
    if (!reverse_uha_available(d, p.w.T))
      return fail(CMCD_ERR_UNSUPPORTED, "no 2nd-order reverse-chain kernel instance for this (target, dim, arch, width=%s%lld)", "", p.w.HP);
    return CMCD_OK;
  }
  if (kind == PLAN_REVERSE_LDVI) {   // `desc` is LDVI's effective descriptor (ldvi_desc): CMCD_MODE_CAIS_UHA_SN = with the network
    if (p.lgcp) return fail(CMCD_ERR_UNSUPPORTED, "the reverse chain has no lgcp kernel%s");
    if (!reverse_ldvi_available(d, p.w.T, d.mode == CMCD_MODE_CAIS_UHA_SN))
      return fail(CMCD_ERR_UNSUPPORTED, "no LDVI reverse-chain kernel instance for this (target, dim, arch, width=%s%lld)", "", p.w.HP);
    p.total = p.need = align4(p.fwd) * 4;
    return CMCD_OK;
  }
  if (kind == PLAN_SEGMENT_LDVI) {   // LDVI's effective descriptor again
    if (p.lgcp) return fail(CMCD_ERR_UNSUPPORTED, "chain segments have no lgcp kernel%s");
    if (!segment_ldvi_available(d, p.w.T, d.mode == CMCD_MODE_CAIS_UHA_SN))
      return fail(CMCD_ERR_UNSUPPORTED, "no LDVI segment kernel instance for this (target, dim, arch, width=%s%lld)", "", p.w.HP);
    p.total = p.need = align4(p.fwd) * 4;
    return CMCD_OK;
  }

  const WsLayout& w = p.w;
  int64_t gws, traj_fl = kept_traj_floats(d, n), scratch_fl = 0;
  if (kind == PLAN_VAR_GRAD) {   // the local (stop_gradient) gradient: no mode check here, the size query answers for any mode
    if (p.lgcp) {                // the reverse launch sequence with z detached, on the trajectory cmcd_bound_var_forward left
      gws = lgcp_grad_workspace_floats(d, n);
    } else {
      const int64_t zs = (int64_t)(d.nbridges + 1) * n * d.dim;
      if (!grad_available(d, w.T)) return fail(CMCD_ERR_UNSUPPORTED, "no gradient kernel instance for this (target, dim, arch, width)%s");
      gws = grad_workspace_floats(d, w.HP, n);
      p.item = grad_item_mode(d, w.T, n);
      // only the work-item path reads the trajectory; without cmcd_bound_var_forward it runs the forward launch sequence
      // once more, with its loss, z and statistics in the scratch
      traj_fl = p.item ? align4(zs) : 0;
      scratch_fl = p.item ? align4(n) + align4(n * d.dim) + 16 : 0;
    }
  } else if (p.lgcp) {           // launch-sequence forward (trajectory kept) + launch-sequence reverse sweep (cmcd_lgcp.hip)
    if (d.mode == CMCD_MODE_CAIS_VAR_SN)
      return fail(CMCD_ERR_UNSUPPORTED, "MCD_CAIS_var_sn: cmcd_grad_workspace_bytes / cmcd_bound_var_forward / cmcd_bound_var_grad_kept%s");
    gws = lgcp_grad_workspace_floats(d, n);
  } else if (d.mode == CMCD_MODE_ULA) {           // no network: the network-free reverse sweep
    if (!ula_grad_available(d)) return fail(CMCD_ERR_UNSUPPORTED, "no MCD_ULA gradient instance for this target%s");
    gws = ula_grad_workspace_floats(d, n);
  } else if (d.mode == CMCD_MODE_CAIS_UHA_SN) {   // (z, rho, rho') kept + its reverse sweep (cmcd_uha.hip)
    if (!uha_grad_available(d, w.T)) return fail(CMCD_ERR_UNSUPPORTED, "no MCD_CAIS_UHA_sn gradient instance for this (target, dim, arch, width)%s");
    gws = uha_grad_workspace_floats(d, w.HP, n);
  } else {
    if ((d.mode != CMCD_MODE_CAIS_SN && d.mode != CMCD_MODE_ULA_SN) || !bptt_available(d, w.T))
      return fail(CMCD_ERR_UNSUPPORTED, query ? "no reparameterised-gradient kernel instance for this (mode, target, dim, arch, width)%s"
                                              : "no reparameterised-gradient kernel instance for this (target, dim, arch, width)%s");
    gws = grad_workspace_floats(d, w.HP, n);
    p.item = grad_item_mode(d, w.T, n);
    traj_fl = align4(traj_fl);
    scratch_fl = p.item ? bptt_item_floats(d, n) : 0;
  }
  p.keep = traj_fl > 0;
  p.gfl = align4(p.fwd);
  p.traj = p.gfl + align4(gws);
  p.scratch = p.traj + traj_fl;
  p.total = p.need = (p.scratch + scratch_fl) * 4;
  if (kind == PLAN_VAR_GRAD && many && !query) {   // the layout is this call's, the demand is the size query's
    CallPlan q;
    make_plan(desc, n, 0, kind, true, q);
    p.need = q.total;
  }
  return CMCD_OK;
}

static int64_t plan_bytes(const cmcd_desc* desc, int64_t n, PlanKind kind) {
  CallPlan p;
  if (check_desc(desc) != CMCD_OK || n < 1 || make_plan(*desc, n, 0, kind, true, p) != CMCD_OK) return 0;
  return p.total;
}

// outer: the plan of the gradient entry point this forward pass belongs to (its trajectory is kept where that plan says)
static int forward_impl(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, int64_t n,
                        const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                        void* workspace, int64_t workspace_bytes, float* out_loss, float* out_z, double* out_stats,
                        void* stream_, bool tables_ready = false, const CallPlan* outer = nullptr) {
  // 1. validate
  const NoiseCapture cap = g_capture;   // armed by cmcd_debug_capture_noise: this call consumes it, whatever happens
  g_capture = NoiseCapture{};
  int rc = check_desc(desc);
  if (rc != CMCD_OK) return rc;
  if ((cap.bits || cap.keys) && desc->target == CMCD_TARGET_LGCP)
    return fail(CMCD_ERR_UNSUPPORTED, "cmcd_debug_capture_noise: trajectory kernels only (not the lgcp launch sequence)%s");
  if (!lay || !seeds || !params || !workspace || !out_loss || !out_z || !out_stats)
    return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  if (n < 1 || n > (int64_t)1 << 31) return fail(CMCD_ERR_BAD_ARG, "n out of range%s");
  const cmcd_desc& d = *desc;
  const int64_t K = d.nbridges, D = d.dim;
  const bool uha = d.mode == CMCD_MODE_CAIS_UHA_SN;

  if (!layout_inside(d, *lay, n_params)) return fail(CMCD_ERR_BAD_ARG, "layout offset missing or outside params_flat%s");
  if ((rc = check_many_gmm(d.target, target_consts, n_target)) != CMCD_OK) return rc;
  if (d.target == CMCD_TARGET_LGCP && (!target_consts || n_target != D * D + D + 3))
    return fail(CMCD_ERR_BAD_ARG, "lgcp needs target_consts = {Kinv[d,d], counts[d], mu0, a, lognorm}%s");

  // 2. plan
  CallPlan own;
  if (!outer) {
    if ((rc = make_plan(d, n, n_target, PLAN_FORWARD, false, own)) != CMCD_OK) return rc;
    outer = &own;
  }
  const CallPlan& p = *outer;
  const cmcd_desc& e = p.d;
  const WsLayout& w = p.w;
  if ((rc = check_workspace(workspace, workspace_bytes, p.fwd * 4)) != CMCD_OK) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* ws = static_cast<float*>(workspace);
  float* traj = p.keep ? ws + p.traj : nullptr;

  // 3. prep.  cmcd_bound_forward_prepared: the caller vouches that the workspace still holds the tables a previous call formed
  // from the SAME (desc, layout, params, target constants, n): the prep launch (4.8 us + a kernel boundary per call) is
  // skipped, and whoever writes the statistics compares the stamp the forming call left (b3[13]; lgcp: sched[0][7]) with
  // this call's (finalize_kernel).  The 2nd-order lgcp sequence has no prepared form.
  const bool ready = tables_ready && !(p.lgcp && uha);
  const uint32_t stamp = tables_stamp(d, *lay, n, n_params, n_target);
  if (!ready) {
    if (p.lgcp) launch_prep_sched(e, *lay, w, params, ws, stream, stamp);   // the rest of lgcp's tables: lgcp_forward
    else launch_prep(e, *lay, w, params, target_consts, p.n_mix, ws, stream, stamp);
  }
  const uint32_t* stamp_slot = ready ? reinterpret_cast<const uint32_t*>(ws + (p.lgcp ? w.sched + 7 : w.b3 + 13)) : nullptr;

  // 4. choose and launch: every branch leaves `records` statistics records at `partials`, or has merged them itself
  double* partials = reinterpret_cast<double*>(ws + w.partials);
  int records = w.n_waves;
  bool merged = false;
  TrajArgs ta{seeds, params, ws, partials, out_loss, out_z, *lay, w, n, (int32_t)K, d.mode == CMCD_MODE_CAIS_VAR_SN ? 1 : 0,
              e.grad_clipping, traj, d.mode == CMCD_MODE_ULA ? 1 : (d.mode == CMCD_MODE_ULA_SN ? 2 : 0)};
  ta.dbg_bits = cap.bits; ta.dbg_keys = cap.keys; ta.dbg_noise = cap.noise;
  if (p.lgcp) {
    snprintf(g_kernel_name, sizeof(g_kernel_name), "%s", lgcp_use_wide(e, n, traj != nullptr)
                 ? "lgcp wide-batch sequence (32x128-tile fp32 GEMM launches)"
                 : "lgcp launch sequence (skinny GEMMs + state kernels)");
    // gradient calls (traj set) hand over the gradient workspace: the forward's consumers keep their activations in its
    // tables, so that the reverse sweep does not recompute them (cmcd_lgcp.hip: lgcp_keep)
    rc = lgcp_forward(e, *lay, w, seeds, n, params, target_consts, ws, out_loss, out_z, &partials, traj, stream_, ready,
                      traj ? ws + p.gfl : nullptr);
    if (rc != CMCD_OK) return fail(rc, "lgcp launch sequence failed%s");
    records = (int)n;
  } else if (uha) {   // 2nd-order CMCD: its own trajectory kernel (cmcd_uha.hip), same prep tables and statistics merge
    rc = uha_forward_launch(e, ta, stream, &records);
    snprintf(g_kernel_name, sizeof(g_kernel_name), "%s", uha_last_kernel_name());
    if (rc != CMCD_OK) return fail(rc, "MCD_CAIS_UHA_sn launch failed%s");
  } else {
    // Kernel variant (desc.reserved: 0 auto, 1 wave-per-tile, 2 CU-cooperative, 3 cooperative on 16-particle tiles,
    // 4 cooperative on 8-particle tiles).  Auto: the cooperative kernel while the batch cannot fill the chip with one
    // wave per tile, on 8-particle tiles while those still get a CU each (n <= 8 x 256).
    const bool coop_ok = coop_available(d, w.T) && d.mode != CMCD_MODE_ULA;
    const bool forced = d.reserved >= 2 && d.reserved <= 5;
    const bool use_coop = forced ? coop_ok : (d.reserved == 1 ? false : (coop_ok && w.n_waves <= coop_max_tiles(d, w.T)));
    if (forced && !coop_ok) return fail(CMCD_ERR_UNSUPPORTED, "no cooperative kernel instance%s");
    const bool half_ok = coop_half_available(d, w.T);
    if ((d.reserved == 4 || d.reserved == 5) && !half_ok) return fail(CMCD_ERR_UNSUPPORTED, "no 8-particle-tile cooperative instance%s");
    const bool half = d.reserved == 4 || d.reserved == 5 || (d.reserved != 3 && half_ok && n <= 8 * 256);
    const bool wide8 = half && d.reserved != 5 && coop_wide8_available(d, w.T);   // d = 10: the dealt-coordinates kernel (5 = the narrow form, A / B)
    if (use_coop) {
      // Small grids (<= 64 workgroups: the launch-bound configurations — gmm / funnel at N = 300 are 38 workgroups): the
      // statistics are merged by the last workgroup to arrive (its counter: the free slot 14 of the b3 row, zeroed by the prep
      // launch of this call) and the finalize launch is dropped: gmm N = 300, K = 8 0.0266 -> 0.0245 ms per call.  Larger
      // grids keep the finalize launch: at the named batch's 250 workgroups the merge tail costs the trajectory kernel what
      // the launch saves (per call 0.2026 vs 0.2024 ms).  Same five doubles bit for bit either way.
      records = int(half ? (n + 7) / 8 : w.n_waves);
      merged = records <= 64;
      if ((rc = profile_begin(stream)) != CMCD_OK) return rc;
      snprintf(g_kernel_name, sizeof(g_kernel_name), "%s<%d-particle tiles%s>", wide8 ? "coop_wide8_kernel" : "coop_kernel",
               half ? 8 : 16, w.T == 9 ? ", 132-wide net" : "");
      if (merged) {
        ta.fin_out = out_stats;
        ta.fin_counter = reinterpret_cast<int32_t*>(ws + w.b3 + 14);
        ta.stamp_slot = stamp_slot;
        ta.stamp_expect = stamp;
      }
      rc = coop_launch(e, ta, half, stream, !wide8);
      if (rc != CMCD_OK) return fail(rc, "cooperative launch failed%s");
    } else if ((rc = traj_launch(e, w, ta, stream, traj_before_launch)) != CMCD_OK) {
      return rc;
    }
    if ((rc = profile_end(stream)) != CMCD_OK) return rc;
  }

  // 5. merge the statistics
  if (!merged) launch_finalize(partials, records, out_stats, stream, stamp_slot, stamp);
  CMCD_HIP_CHECK(hipGetLastError());
  return CMCD_OK;
}

// The arguments every reverse and segment entry point (and cmcd_ldvi_bound_grad) has in common, as the caller gave them
struct ChainArgs {
  const int32_t* seeds;
  int64_t n;
  const float* params;
  int64_t n_params;
  const float* target_consts;
  int64_t n_target;
  void* workspace;
  int64_t workspace_bytes;
  void* stream_;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* ws() const { return static_cast<float*>(workspace); }
  double* partials(const WsLayout& w) const { return reinterpret_cast<double*>(ws() + w.partials); }
};

// What cmcd_bound_reverse and cmcd_bound_segment do between their own argument checks and their kernel launch, in this order:
// plan (refuses the modes and targets without an instance before the layout is looked at), layout, many_gmm constants,
// workspace, the prep launch (the forward call's tables, formed by the same launch, on every call), and the TrajArgs of a
// wave-per-tile launch with one statistics record per 16-particle tile.
static int chain_call_begin(const cmcd_desc& d, const cmcd_layout* lay, PlanKind kind, const ChainArgs& a, float* out_loss,
                            float* out_z, CallPlan& p, TrajArgs& ta) {
  int rc;
  if ((rc = make_plan(d, a.n, a.n_target, kind, false, p)) != CMCD_OK) return rc;
  if (!layout_inside(d, *lay, a.n_params)) return fail(CMCD_ERR_BAD_ARG, "layout offset missing or outside params_flat%s");
  if ((rc = check_many_gmm(d.target, a.target_consts, a.n_target)) != CMCD_OK) return rc;
  if ((rc = check_workspace(a.workspace, a.workspace_bytes, p.need)) != CMCD_OK) return rc;
  launch_prep(p.d, *lay, p.w, a.params, a.target_consts, p.n_mix, a.ws(), a.stream,
              tables_stamp(d, *lay, a.n, a.n_params, a.n_target));
  ta = TrajArgs{a.seeds, a.params, a.ws(), a.partials(p.w), out_loss, out_z, *lay, p.w, a.n, (int32_t)d.nbridges,
                d.mode == CMCD_MODE_CAIS_VAR_SN ? 1 : 0, p.d.grad_clipping, nullptr,
                d.mode == CMCD_MODE_ULA ? 1 : (d.mode == CMCD_MODE_ULA_SN ? 2 : 0)};
  return CMCD_OK;
}

// ... and behind the launch of every reverse and segment call (LDVI's forward and gradient call too): merge the `records`
// statistics records the kernel left at `partials`, one per 16-particle tile
static int chain_call_end(const double* partials, int64_t records, double* out_stats, hipStream_t stream) {
  launch_finalize(partials, (int32_t)records, out_stats, stream, nullptr, 0u);
  CMCD_HIP_CHECK(hipGetLastError());
  return CMCD_OK;
}

// the checks of every segment call on [k0, k1) and the seeds
static int segment_range(int32_t k0, int32_t k1, int32_t nbridges, const int32_t* seeds) {
  if (k0 < 0 || k0 >= k1 || k1 > nbridges)
    return fail(CMCD_ERR_BAD_ARG, "segment bridges must satisfy 0 <= k0 < k1 <= nbridges (got k1 = %s%lld)", "", k1);
  if (k0 == 0 && !seeds) return fail(CMCD_ERR_BAD_ARG, "a segment that starts at bridge 0 needs seeds%s");
  return CMCD_OK;
}

// the reverse-time chain: x[n][dim] target draws -> out_w, out_z0, statistics over l := w (cmcd_reverse.hip).
// uha: the 2nd-order chain, which also returns the end momentum out_rho0 (cmcd_reverse_uha.hip)
static int reverse_impl(const cmcd_desc* desc, const cmcd_layout* lay, const ChainArgs& a, const float* x, float* out_w,
                        float* out_z0, float* out_rho0, double* out_stats, bool uha) {
  int rc = check_desc(desc);
  if (rc != CMCD_OK) return rc;
  if (!lay || !a.seeds || !x || !a.params || !a.workspace || !out_w || !out_z0 || (uha && !out_rho0) || !out_stats)
    return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  if (a.n < 1 || a.n > (int64_t)1 << 31) return fail(CMCD_ERR_BAD_ARG, "n out of range%s");
  CallPlan p;
  TrajArgs ta;
  if ((rc = chain_call_begin(*desc, lay, uha ? PLAN_REVERSE_UHA : PLAN_REVERSE, a, out_w, out_z0, p, ta)) != CMCD_OK) return rc;
  snprintf(g_kernel_name, sizeof(g_kernel_name), uha ? "reverse_uha_kernel" : "reverse_traj_kernel");
  rc = uha ? reverse_uha_launch(p.d, p.w, ta, x, out_rho0, a.stream) : reverse_launch(p.d, p.w, ta, x, a.stream);
  if (rc != CMCD_OK) return rc;
  return chain_call_end(ta.partials, ta.w.n_waves, out_stats, a.stream);
}

// bridges [k0, k1) of the forward chain from the state (z, wpath, key); seeds are read when k0 == 0 (cmcd_segment.hip).
// uha: the 2nd-order chain from (z, rho, wpath, key) (cmcd_segment_uha.hip)
static int segment_impl(const cmcd_desc* desc, const cmcd_layout* lay, int32_t k0, int32_t k1, const ChainArgs& a, float* z,
                        float* rho, float* wpath, uint32_t* key, float* out_lg, double* out_stats, bool uha) {
  int rc = check_desc(desc);
  if (rc != CMCD_OK) return rc;
  if (!lay || !a.params || !a.workspace || !z || (uha && !rho) || !wpath || !key || !out_lg || !out_stats)
    return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  if (a.n < 1 || a.n > (int64_t)1 << 31) return fail(CMCD_ERR_BAD_ARG, "n out of range%s");
  if ((rc = segment_range(k0, k1, desc->nbridges, a.seeds)) != CMCD_OK) return rc;
  CallPlan p;
  TrajArgs ta;
  if ((rc = chain_call_begin(*desc, lay, uha ? PLAN_SEGMENT_UHA : PLAN_SEGMENT, a, nullptr, nullptr, p, ta)) != CMCD_OK) return rc;
  snprintf(g_kernel_name, sizeof(g_kernel_name), uha ? "segment_uha_kernel" : "segment_traj_kernel");
  rc = uha ? segment_uha_launch(p.d, p.w, ta, k0, k1, z, rho, wpath, key, out_lg, a.stream)
           : segment_launch(p.d, p.w, ta, k0, k1, z, wpath, key, out_lg, a.stream);
  if (rc != CMCD_OK) return rc;
  return chain_call_end(ta.partials, ta.w.n_waves, out_stats, a.stream);
}

// the VarGrad gradient on the tables (and, for work items and lgcp, the trajectory) in the workspace; kept: left there by
// cmcd_bound_var_forward, otherwise formed here
static int var_grad_impl(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, int64_t n,
                         const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                         const float* omega, void* workspace, int64_t workspace_bytes, float* grad, bool kept,
                         void* stream_) {
  int rc = check_desc(desc);
  if (rc != CMCD_OK) return rc;
  if (!lay || !seeds || !params || !omega || !workspace || !grad) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  if (desc->mode != CMCD_MODE_CAIS_VAR_SN)
    return fail(CMCD_ERR_UNSUPPORTED, "the local (stop_gradient) gradient exists for MCD_CAIS_var_sn only%s");
  const cmcd_desc& d = *desc;
  if (d.target == CMCD_TARGET_LGCP && !kept)
    return fail(CMCD_ERR_UNSUPPORTED, "lgcp: call cmcd_bound_var_forward, then cmcd_bound_var_grad_kept on the same workspace%s");
  if ((rc = check_many_gmm(d.target, target_consts, n_target)) != CMCD_OK) return rc;
  CallPlan p;
  if ((rc = make_plan(d, n, n_target, PLAN_VAR_GRAD, false, p)) != CMCD_OK) return rc;
  if ((rc = check_workspace(workspace, workspace_bytes, p.need)) != CMCD_OK) return rc;
  float* ws = static_cast<float*>(workspace);
  float* traj = p.keep ? ws + p.traj : nullptr;
  if (p.lgcp) {
    rc = lgcp_grad(d, *lay, p.w, n, params, n_params, target_consts, ws, traj, ws + p.gfl, 0.f, omega, false, grad, stream_);
    return rc != CMCD_OK ? fail(rc, "lgcp gradient launch sequence failed%s") : CMCD_OK;
  }
  if (p.item && !kept) {   // the forward launch sequence once more, keeping z_0..z_K
    float* sl = ws + p.scratch;
    float* sz = sl + align4(n);
    double* sst = reinterpret_cast<double*>(sz + align4(n * d.dim));
    rc = forward_impl(desc, lay, seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, sl, sz, sst,
                      stream_, false, &p);
    if (rc != CMCD_OK) return rc;
  } else if (!kept) {
    launch_prep(p.d, *lay, p.w, params, target_consts, p.n_mix, ws, static_cast<hipStream_t>(stream_),
                tables_stamp(d, *lay, n, n_params, n_target));
  }
  rc = grad_launch(d, *lay, p.w, seeds, n, params, n_params, ws, omega, 0.f, false, p.item, traj, nullptr, ws + p.gfl, grad,
                   stream_);
  return rc != CMCD_OK ? fail(rc, "gradient launch failed%s") : CMCD_OK;
}

}  // namespace cmcd

using namespace cmcd;

extern "C" {

int cmcd_version(void) { return CMCD_ABI_VERSION; }
const char* cmcd_last_error(void) { return g_err; }

int64_t cmcd_target_floats(const cmcd_desc* desc, int32_t n_mixes) {
  if (!desc) return -1;
  switch (desc->target) {
    case CMCD_TARGET_GMM:
    case CMCD_TARGET_FUNNEL: return 0;
    case CMCD_TARGET_MANY_GMM: return 1 + 2 * (int64_t)n_mixes;
    case CMCD_TARGET_LGCP: return (int64_t)desc->dim * desc->dim + desc->dim + 3;
    default: return -1;
  }
}

int64_t cmcd_workspace_bytes(const cmcd_desc* desc, int64_t n) { return plan_bytes(desc, n, PLAN_FORWARD); }
int64_t cmcd_grad_workspace_bytes(const cmcd_desc* desc, int64_t n) { return plan_bytes(desc, n, PLAN_VAR_GRAD); }
int64_t cmcd_bound_grad_workspace_bytes(const cmcd_desc* desc, int64_t n) { return plan_bytes(desc, n, PLAN_BOUND_GRAD); }

int cmcd_bound_forward(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, int64_t n,
                       const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                       void* workspace, int64_t workspace_bytes, float* out_loss, float* out_z,
                       double* out_stats, void* stream_) {
  return forward_impl(desc, lay, seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes,
                      out_loss, out_z, out_stats, stream_);
}

int cmcd_bound_forward_prepared(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, int64_t n,
                                const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                                void* workspace, int64_t workspace_bytes, float* out_loss, float* out_z,
                                double* out_stats, void* stream_) {
  return forward_impl(desc, lay, seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes,
                      out_loss, out_z, out_stats, stream_, true);
}

int64_t cmcd_reverse_workspace_bytes(const cmcd_desc* desc, int64_t n) { return plan_bytes(desc, n, PLAN_REVERSE); }

int cmcd_bound_reverse(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, const float* x, int64_t n,
                       const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                       void* workspace, int64_t workspace_bytes, float* out_w, float* out_z0, double* out_stats,
                       void* stream_) {
  return reverse_impl(desc, lay, {seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, stream_}, x, out_w, out_z0,
                      nullptr, out_stats, false);
}

int64_t cmcd_reverse_uha_workspace_bytes(const cmcd_desc* desc, int64_t n) { return plan_bytes(desc, n, PLAN_REVERSE_UHA); }

int cmcd_bound_reverse_uha(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, const float* x, int64_t n,
                           const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                           void* workspace, int64_t workspace_bytes, float* out_w, float* out_z0, float* out_rho0,
                           double* out_stats, void* stream_) {
  return reverse_impl(desc, lay, {seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, stream_}, x, out_w, out_z0,
                      out_rho0, out_stats, true);
}

int64_t cmcd_segment_workspace_bytes(const cmcd_desc* desc, int64_t n) { return plan_bytes(desc, n, PLAN_SEGMENT); }

int cmcd_bound_segment(const cmcd_desc* desc, const cmcd_layout* lay, int32_t k0, int32_t k1, const int32_t* seeds, int64_t n,
                       const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                       void* workspace, int64_t workspace_bytes, float* z_inout, float* wpath_inout, uint32_t* key_inout,
                       float* out_lg, double* out_stats, void* stream_) {
  return segment_impl(desc, lay, k0, k1, {seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, stream_},
                      z_inout, nullptr, wpath_inout, key_inout, out_lg, out_stats, false);
}

int64_t cmcd_segment_uha_workspace_bytes(const cmcd_desc* desc, int64_t n) { return plan_bytes(desc, n, PLAN_SEGMENT_UHA); }

int cmcd_bound_segment_uha(const cmcd_desc* desc, const cmcd_layout* lay, int32_t k0, int32_t k1, const int32_t* seeds, int64_t n,
                           const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                           void* workspace, int64_t workspace_bytes, float* z_inout, float* rho_inout, float* wpath_inout,
                           uint32_t* key_inout, float* out_lg, double* out_stats, void* stream_) {
  return segment_impl(desc, lay, k0, k1, {seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, stream_},
                      z_inout, rho_inout, wpath_inout, key_inout, out_lg, out_stats, true);
}

int cmcd_bound_grad(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, int64_t n,
                    const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                    float omega, void* workspace, int64_t workspace_bytes, float* out_loss, float* out_z,
                    double* out_stats, float* grad, void* stream_) {
  int rc = check_desc(desc);
  if (rc != CMCD_OK) return rc;
  if (!grad) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  if (desc->mode != CMCD_MODE_CAIS_SN && desc->mode != CMCD_MODE_ULA_SN && desc->mode != CMCD_MODE_ULA &&
      desc->mode != CMCD_MODE_CAIS_UHA_SN)
    return fail(CMCD_ERR_UNSUPPORTED, "the reparameterised gradient exists for MCD_CAIS_sn, MCD_CAIS_UHA_sn and MCD_ULA[_sn] (MCD_CAIS_var_sn: cmcd_bound_var_grad)%s");
  CallPlan p;
  if ((rc = make_plan(*desc, n, n_target, PLAN_BOUND_GRAD, false, p)) != CMCD_OK) return rc;
  if ((rc = check_workspace(workspace, workspace_bytes, p.need)) != CMCD_OK) return rc;
  // forward with the trajectory kept, then the reverse sweep of the mode
  rc = forward_impl(desc, lay, seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, out_loss,
                    out_z, out_stats, stream_, false, &p);
  if (rc != CMCD_OK) return rc;
  const cmcd_desc& d = p.d;
  float* ws = static_cast<float*>(workspace);
  float* traj = ws + p.traj;
  float* gws = ws + p.gfl;
  if (p.lgcp) {
    rc = lgcp_grad(d, *lay, p.w, n, params, n_params, target_consts, ws, traj, gws, omega, nullptr, true, grad, stream_);
    return rc != CMCD_OK ? fail(rc, "lgcp gradient launch sequence failed%s") : CMCD_OK;
  }
  if (d.mode == CMCD_MODE_ULA)
    rc = ula_grad_launch(d, *lay, p.w, n, params, n_params, ws, traj, gws, omega, grad, stream_);
  else if (d.mode == CMCD_MODE_CAIS_UHA_SN)
    rc = uha_grad_launch(d, *lay, p.w, n, params, n_params, ws, traj, gws, omega, grad, stream_);
  else
    rc = grad_launch(d, *lay, p.w, seeds, n, params, n_params, ws, nullptr, omega, true, p.item, traj,
                     p.item ? ws + p.scratch : nullptr, gws, grad, stream_);
  return rc != CMCD_OK ? fail(rc, "gradient launch failed%s") : CMCD_OK;
}

// LDVI (cmcd_ldvi.hip).  The caller's descriptor with what the mode fixes: the network and its tables are those of
// CMCD_MODE_CAIS_UHA_SN on the geffner net (same workspace plan, same prep launch); without a network the schedule tables and
// target constants of CMCD_MODE_ULA.  Order of refusals: descriptor / lgcp / dds / the descriptor's own checks / instance /
// K, then (entry point) pointers, n, layout, target constants, workspace.
static int ldvi_desc(const cmcd_desc* desc, int32_t use_net, cmcd_desc& e) {
  if (!desc) return fail(CMCD_ERR_BAD_ARG, "null desc%s");
  if (desc->target == CMCD_TARGET_LGCP)
    return fail(CMCD_ERR_UNSUPPORTED, "LDVI (MCD_U_a-lp[-sn]) on lgcp is not implemented (no launch sequence for d = 1600)%s");
  if (use_net && desc->arch != CMCD_ARCH_GEFFNER)
    return fail(CMCD_ERR_UNSUPPORTED, "LDVI (MCD_U_a-lp-sn): nn_arch dds is not implemented (geffner only)%s");
  e = *desc;
  e.mode = use_net ? CMCD_MODE_CAIS_UHA_SN : CMCD_MODE_ULA;
  if (!use_net) e.arch = CMCD_ARCH_DDS;   // MCD_ULA's placeholder: no network
  e.eps_schedule = CMCD_EPS_CONST;
  e.grad_clipping = 0;
  e.reserved = 0;
  int rc = check_desc(&e);
  if (rc != CMCD_OK) return rc;
  int HP = 0;
  hidden_width(e, HP);
  if (!ldvi_available(e, HP / 16, use_net != 0))
    return fail(CMCD_ERR_UNSUPPORTED, "no LDVI kernel instance for this (target, dim, width=%s%lld)", "", HP);
  if (e.nbridges > 4096) return fail(CMCD_ERR_UNSUPPORTED, "LDVI: nbridges above 4096%s");
  return CMCD_OK;
}

// bytes of an LDVI workspace: the plan's forward part (PLAN_REVERSE_LDVI / PLAN_SEGMENT_LDVI: their total), then the gradient
// workspace of cmcd_ldvi_bound_grad
static int64_t ldvi_bytes(const cmcd_desc& e, const CallPlan& p, int64_t n, bool use_net, bool with_grad) {
  return (align4(p.fwd) + (with_grad ? ldvi_grad_floats(e, p.w.HP, n, use_net) : 0)) * 4;
}

// the three LDVI size queries: 0 for whatever ldvi_desc or the plan of `kind` refuses
static int64_t ldvi_query(const cmcd_desc* desc, int32_t use_net, int64_t n, PlanKind kind, bool with_grad) {
  cmcd_desc e;
  CallPlan p;
  if (ldvi_desc(desc, use_net, e) != CMCD_OK || n < 1 || n > (int64_t)1 << 31) return 0;
  if (make_plan(e, n, 0, kind, true, p) != CMCD_OK) return 0;
  return ldvi_bytes(e, p, n, use_net != 0, with_grad);
}

// What the three LDVI calls do in front of their launch, chain_call_begin's sibling for a descriptor that ldvi_desc forms:
// descriptor, null pointers (lay, params and workspace here; other_null: the rest of the entry point's own list), n, for a
// segment its range = {k0, k1}, layout with the gamma leaf, many_gmm constants, the plan of this call (layout) and of its size
// query (demand: many_gmm's largest target block), workspace, the prep launch.  -> the effective descriptor and the plan.
static int ldvi_call_begin(const cmcd_desc* desc, int32_t use_net, const cmcd_layout* lay, const ChainArgs& a, bool other_null,
                           const int32_t* range, PlanKind kind, bool with_grad, cmcd_desc& e, CallPlan& p) {
  int rc = ldvi_desc(desc, use_net, e);
  if (rc != CMCD_OK) return rc;
  if (!lay || !a.params || !a.workspace || other_null) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  if (a.n < 1 || a.n > (int64_t)1 << 31) return fail(CMCD_ERR_BAD_ARG, "n out of range%s");
  if (range && (rc = segment_range(range[0], range[1], e.nbridges, a.seeds)) != CMCD_OK) return rc;
  if (!layout_inside(e, *lay, a.n_params) || lay->gamma < 0 || lay->gamma >= a.n_params)
    return fail(CMCD_ERR_BAD_ARG, "layout offset missing or outside params_flat%s");
  if ((rc = check_many_gmm(e.target, a.target_consts, a.n_target)) != CMCD_OK) return rc;
  CallPlan q;
  if ((rc = make_plan(e, a.n, a.n_target, kind, false, p)) != CMCD_OK) return rc;
  if ((rc = make_plan(e, a.n, 0, kind, true, q)) != CMCD_OK) return rc;
  p.need = ldvi_bytes(e, q, a.n, use_net != 0, with_grad);
  if ((rc = check_workspace(a.workspace, a.workspace_bytes, p.need)) != CMCD_OK) return rc;
  launch_prep(e, *lay, p.w, a.params, a.target_consts, p.n_mix, a.ws(), a.stream, tables_stamp(e, *lay, a.n, a.n_params, a.n_target));
  return CMCD_OK;
}

int64_t cmcd_ldvi_workspace_bytes(const cmcd_desc* desc, int32_t use_net, int64_t n, int32_t with_grad) {
  return ldvi_query(desc, use_net, n, PLAN_FORWARD, with_grad != 0);
}

int cmcd_ldvi_bound_grad(const cmcd_desc* desc, const cmcd_layout* lay, int32_t use_net, const int32_t* seeds, int64_t n,
                         const float* params, int64_t n_params, const float* target_consts, int64_t n_target, float omega,
                         void* workspace, int64_t workspace_bytes, float* out_loss, float* out_z, double* out_stats,
                         float* grad, void* stream_) {
  const ChainArgs a{seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, stream_};
  cmcd_desc e;
  CallPlan p;
  int rc = ldvi_call_begin(desc, use_net, lay, a, !seeds || !out_loss || !out_z || !out_stats, nullptr, PLAN_FORWARD, grad != nullptr,
                           e, p);
  if (rc != CMCD_OK) return rc;
  rc = ldvi_launch(e, *lay, p.w, use_net != 0, seeds, n, params, n_params, a.ws(), a.ws() + align4(p.fwd), omega, out_loss, out_z,
                   grad, a.stream);
  if (rc != CMCD_OK) return rc;
  return chain_call_end(a.partials(p.w), p.w.n_waves, out_stats, a.stream);
}

// ---- the reverse-time chains of the two momentum baselines (cmcd_reverse_ldvi.hip, cmcd_reverse_hais.hip)
int64_t cmcd_reverse_ldvi_workspace_bytes(const cmcd_desc* desc, int32_t use_net, int64_t n) {
  return ldvi_query(desc, use_net, n, PLAN_REVERSE_LDVI, false);
}

int cmcd_bound_reverse_ldvi(const cmcd_desc* desc, const cmcd_layout* lay, int32_t use_net, const int32_t* seeds, const float* x,
                            int64_t n, const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                            void* workspace, int64_t workspace_bytes, float* out_w, float* out_z0, float* out_rho0,
                            double* out_stats, void* stream_) {
  const ChainArgs a{seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, stream_};
  cmcd_desc e;
  CallPlan p;
  int rc = ldvi_call_begin(desc, use_net, lay, a, !seeds || !x || !out_w || !out_z0 || !out_rho0 || !out_stats, nullptr,
                           PLAN_REVERSE_LDVI, false, e, p);
  if (rc != CMCD_OK) return rc;
  snprintf(g_kernel_name, sizeof(g_kernel_name), "reverse_ldvi_kernel");
  rc = reverse_ldvi_launch(e, *lay, p.w, use_net != 0, seeds, x, n, params, a.ws(), out_w, out_z0, out_rho0, a.stream);
  if (rc != CMCD_OK) return rc;
  return chain_call_end(a.partials(p.w), p.w.n_waves, out_stats, a.stream);
}

// UHA has no descriptor and no prep tables: its plan is the refusals of cmcd_hais_workspace_bytes, in that order, and one
// statistics record per tile.  The reverse and the segment call differ in their kernel instances and in their words for lgcp
// and for a missing instance.
struct HaisChain {
  bool (*available)(int target, int dim);
  const char* no_lgcp;
  const char* no_instance;
};
static const HaisChain kReverseHais = {reverse_hais_available,
                                       "the reverse chain of UHA has no lgcp kernel (lgcp has no exact target draws)%s",
                                       "no Hamiltonian AIS reverse-chain kernel instance for this (target, dim)%s"};
static const HaisChain kSegmentHais = {segment_hais_available,
                                       "chain segments of UHA have no lgcp kernel (cmcd_hais_lgcp.hip runs whole chains)%s",
                                       "no Hamiltonian AIS segment kernel instance for this (target, dim)%s"};
struct HaisShape { int32_t target, dim, nbridges, lfsteps; };   // what stands for a descriptor in the UHA calls

// -> CMCD_OK and the workspace floats, or the refusal with cmcd_last_error set
static int hais_chain_plan(const HaisChain& c, const HaisShape& s, int64_t n, int64_t& floats) {
  floats = 0;
  if (s.nbridges < 1 || s.lfsteps < 1) return fail(CMCD_ERR_BAD_ARG, "nbridges and lfsteps must be >= 1%s");
  if (n < 1 || n > (int64_t)1 << 31 || s.dim < 1) return fail(CMCD_ERR_BAD_ARG, "n or dim out of range%s");
  if (s.target == CMCD_TARGET_LGCP) return fail(CMCD_ERR_UNSUPPORTED, c.no_lgcp);
  if (!c.available(s.target, s.dim)) return fail(CMCD_ERR_UNSUPPORTED, c.no_instance);
  if (!reverse_hais_shape_ok(s.nbridges, s.lfsteps, n))
    return fail(CMCD_ERR_UNSUPPORTED, "nbridges above 4096 or nbridges * lfsteps above 2^24%s");
  floats = reverse_hais_floats(n);
  return CMCD_OK;
}

static int64_t hais_chain_query(const HaisChain& c, const HaisShape& s, int64_t n) {
  int64_t floats;
  return hais_chain_plan(c, s, n, floats) == CMCD_OK ? floats * 4 : 0;
}

// What cmcd_bound_reverse_hais and cmcd_bound_segment_hais do in front of their launch: null pointers (lay, params and
// workspace here; other_null: the rest of the entry point's own list), the plan, for a segment its range = {k0, k1}, the layout,
// many_gmm constants (-> n_mix), workspace.
// (cmcd_hais.hip and cmcd_hais_lgcp.hip keep their own copies of the cmcd_hais_layout check: kernel files, their own entry points.)
static int hais_chain_begin(const HaisChain& c, const HaisShape& s, const cmcd_hais_layout* lay, const ChainArgs& a, bool other_null,
                            const int32_t* range, int& n_mix) {
  if (!lay || !a.params || !a.workspace || other_null) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  int64_t floats;
  int rc = hais_chain_plan(c, s, a.n, floats);
  if (rc != CMCD_OK) return rc;
  if (range && (rc = segment_range(range[0], range[1], s.nbridges, a.seeds)) != CMCD_OK) return rc;
  if (lay->ngrid < 0 || lay->ngrid > 1024) return fail(CMCD_ERR_BAD_ARG, "ngrid out of range (0 .. 1024)%s");
  auto inside = [&](int64_t off, int64_t len) { return off >= 0 && off + len <= a.n_params; };
  if (!(inside(lay->vd_mean, s.dim) && inside(lay->vd_logdiag, s.dim) && inside(lay->eps, 1) && inside(lay->eta, 1) &&
        inside(lay->md, s.dim) && inside(lay->mgridref_y, lay->ngrid + 1) && inside(lay->gridref_x, lay->ngrid + 2) &&
        inside(lay->target_x, s.nbridges)))
    return fail(CMCD_ERR_BAD_ARG, "layout offset missing or outside params_flat%s");
  if ((rc = check_many_gmm(s.target, a.target_consts, a.n_target, &n_mix)) != CMCD_OK) return rc;
  return check_workspace(a.workspace, a.workspace_bytes, floats * 4);
}

int64_t cmcd_reverse_hais_workspace_bytes(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, int64_t n) {
  return hais_chain_query(kReverseHais, {target, dim, nbridges, lfsteps}, n);
}

int cmcd_bound_reverse_hais(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout* lay,
                            const int32_t* seeds, const float* x, int64_t n, const float* params, int64_t n_params,
                            const float* target_consts, int64_t n_target, void* workspace, int64_t workspace_bytes, float* out_w,
                            float* out_z0, float* out_rho0, double* out_stats, void* stream_) {
  const ChainArgs a{seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, stream_};
  int n_mix = 0;
  int rc = hais_chain_begin(kReverseHais, {target, dim, nbridges, lfsteps}, lay, a,
                            !seeds || !x || !out_w || !out_z0 || !out_rho0 || !out_stats, nullptr, n_mix);
  if (rc != CMCD_OK) return rc;
  snprintf(g_kernel_name, sizeof(g_kernel_name), "reverse_hais_kernel");
  rc = reverse_hais_launch(target, dim, nbridges, lfsteps, *lay, seeds, x, n, params, target_consts, n_mix, a.ws(), out_w, out_z0,
                           out_rho0, a.stream);
  if (rc != CMCD_OK) return rc;
  return chain_call_end(reinterpret_cast<double*>(workspace), (n + 15) / 16, out_stats, a.stream);
}

// ---- chain segments of the two momentum baselines (cmcd_segment_ldvi.hip, cmcd_segment_hais.hip): the plans, the layouts and
// the refusals of their reverse chains, with segment_range's checks on [k0, k1) and the seeds
int64_t cmcd_segment_ldvi_workspace_bytes(const cmcd_desc* desc, int32_t use_net, int64_t n) {
  return ldvi_query(desc, use_net, n, PLAN_SEGMENT_LDVI, false);
}

int cmcd_bound_segment_ldvi(const cmcd_desc* desc, const cmcd_layout* lay, int32_t use_net, int32_t k0, int32_t k1,
                            const int32_t* seeds, int64_t n, const float* params, int64_t n_params, const float* target_consts,
                            int64_t n_target, void* workspace, int64_t workspace_bytes, float* z_inout, float* rho_inout,
                            float* wpath_inout, uint32_t* key_inout, float* out_lg, double* out_stats, void* stream_) {
  const ChainArgs a{seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, stream_};
  const int32_t range[2] = {k0, k1};
  cmcd_desc e;
  CallPlan p;
  int rc = ldvi_call_begin(desc, use_net, lay, a, !z_inout || !rho_inout || !wpath_inout || !key_inout || !out_lg || !out_stats, range,
                           PLAN_SEGMENT_LDVI, false, e, p);
  if (rc != CMCD_OK) return rc;
  snprintf(g_kernel_name, sizeof(g_kernel_name), "segment_ldvi_kernel");
  rc = segment_ldvi_launch(e, *lay, p.w, use_net != 0, k0, k1, seeds, n, params, a.ws(), z_inout, rho_inout, wpath_inout, key_inout,
                           out_lg, a.stream);
  if (rc != CMCD_OK) return rc;
  return chain_call_end(a.partials(p.w), p.w.n_waves, out_stats, a.stream);
}

int64_t cmcd_segment_hais_workspace_bytes(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, int64_t n) {
  return hais_chain_query(kSegmentHais, {target, dim, nbridges, lfsteps}, n);
}

int cmcd_bound_segment_hais(int32_t target, int32_t dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout* lay, int32_t k0,
                            int32_t k1, const int32_t* seeds, int64_t n, const float* params, int64_t n_params,
                            const float* target_consts, int64_t n_target, void* workspace, int64_t workspace_bytes, float* z_inout,
                            float* rho_inout, float* wpath_inout, uint32_t* key_inout, float* out_lg, double* out_stats,
                            void* stream_) {
  const ChainArgs a{seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, stream_};
  const int32_t range[2] = {k0, k1};
  int n_mix = 0;
  int rc = hais_chain_begin(kSegmentHais, {target, dim, nbridges, lfsteps}, lay, a,
                            !z_inout || !rho_inout || !wpath_inout || !key_inout || !out_lg || !out_stats, range, n_mix);
  if (rc != CMCD_OK) return rc;
  snprintf(g_kernel_name, sizeof(g_kernel_name), "segment_hais_kernel");
  rc = segment_hais_launch(target, dim, nbridges, lfsteps, *lay, k0, k1, seeds, n, params, target_consts, n_mix, a.ws(), z_inout,
                           rho_inout, wpath_inout, key_inout, out_lg, a.stream);
  if (rc != CMCD_OK) return rc;
  return chain_call_end(reinterpret_cast<double*>(workspace), (n + 15) / 16, out_stats, a.stream);
}

int cmcd_vargrad_weights(const float* loss, const double* stats, int64_t n, int64_t n_total, float* omega,
                         void* stream_) {
  if (!loss || !stats || !omega || n < 1 || n_total < n) return fail(CMCD_ERR_BAD_ARG, "bad argument%s");
  launch_vargrad_weights(loss, stats, n, n_total, omega, static_cast<hipStream_t>(stream_));
  CMCD_HIP_CHECK(hipGetLastError());
  return CMCD_OK;
}

int cmcd_bound_var_grad(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, int64_t n,
                        const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                        const float* omega, void* workspace, int64_t workspace_bytes, float* grad, void* stream_) {
  return var_grad_impl(desc, lay, seeds, n, params, n_params, target_consts, n_target, omega, workspace,
                       workspace_bytes, grad, false, stream_);
}

int cmcd_bound_var_forward(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, int64_t n,
                           const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                           void* workspace, int64_t workspace_bytes, float* out_loss, float* out_z,
                           double* out_stats, void* stream_) {
  int rc = check_desc(desc);
  if (rc != CMCD_OK) return rc;
  if (desc->mode != CMCD_MODE_CAIS_VAR_SN)
    return fail(CMCD_ERR_UNSUPPORTED, "the local (stop_gradient) gradient exists for MCD_CAIS_var_sn only%s");
  CallPlan p;   // (no gradient instance, or no particles: the size query answers 0)
  if (n < 1 || make_plan(*desc, n, n_target, PLAN_VAR_GRAD, false, p) != CMCD_OK) return CMCD_ERR_UNSUPPORTED;
  if ((rc = check_workspace(workspace, workspace_bytes, p.need)) != CMCD_OK) return rc;
  return forward_impl(desc, lay, seeds, n, params, n_params, target_consts, n_target, workspace, workspace_bytes, out_loss,
                      out_z, out_stats, stream_, false, &p);
}

int cmcd_bound_var_grad_kept(const cmcd_desc* desc, const cmcd_layout* lay, const int32_t* seeds, int64_t n,
                             const float* params, int64_t n_params, const float* target_consts, int64_t n_target,
                             const float* omega, void* workspace, int64_t workspace_bytes, float* grad,
                             void* stream_) {
  return var_grad_impl(desc, lay, seeds, n, params, n_params, target_consts, n_target, omega, workspace,
                       workspace_bytes, grad, true, stream_);
}

int cmcd_stats_merge_device(const double* rows, int32_t count, double* out5, void* stream_) {
  if (!rows || !out5 || count < 1) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  launch_finalize(rows, count, out5, static_cast<hipStream_t>(stream_), nullptr, 0u);
  CMCD_HIP_CHECK(hipGetLastError());
  return CMCD_OK;
}

int cmcd_stats_merge(const double* stats, const int64_t* n_per, int32_t count, double* merged5, double* out3) {
  if (!stats || !n_per || count < 1 || !merged5 || !out3) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  double acc[CMCD_NSTATS] = {0, 0, 0, -INFINITY, 0};
  int64_t n = 0;
  for (int i = 0; i < count; ++i) {
    const double* b = stats + (int64_t)i * CMCD_NSTATS;
    acc[0] += b[0]; acc[1] += b[1]; acc[2] += b[2];
    const double m = fmax(acc[3], b[3]);
    const double sa = (acc[3] > -INFINITY && m < INFINITY) ? acc[4] * exp(acc[3] - m) : (acc[3] == m ? acc[4] : 0.0);
    const double sb = (b[3] > -INFINITY && m < INFINITY) ? b[4] * exp(b[3] - m) : (b[3] == m ? b[4] : 0.0);
    acc[3] = m; acc[4] = sa + sb;
    n += n_per[i];
  }
  if (n < 1) return fail(CMCD_ERR_BAD_ARG, "no particles%s");
  memcpy(merged5, acc, sizeof(acc));
  const double mean = acc[1] / (double)n;
  out3[0] = mean;
  out3[1] = acc[2] / (double)n - mean * mean;        // var(ddof=0); inf - inf = NaN like the reference
  out3[2] = acc[3] + log(acc[4]) - log((double)n);   // logsumexp(-l) - log n
  return CMCD_OK;
}

int64_t cmcd_resample_workspace_bytes(int64_t n, int32_t groups) {
  if (n < 1 || n > INT32_MAX || groups < 1 || n % groups != 0 || n / groups > kResampleMaxGroup) return 0;
  return resample_workspace_bytes(n);
}

int cmcd_resample_systematic(const float* loss, const float* z, int64_t n, int32_t dim, int32_t groups, uint32_t seed,
                             void* workspace, int64_t workspace_bytes, int32_t* out_index, float* out_z, double* out_stats,
                             void* stream_) {
  if (!loss || !out_stats) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  if (n < 1 || n > INT32_MAX) return fail(CMCD_ERR_BAD_ARG, "n out of range%s");   // out_index holds int32 row numbers
  if (groups < 1) return fail(CMCD_ERR_BAD_ARG, "groups must be >= 1%s");
  if (n % groups != 0) return fail(CMCD_ERR_BAD_ARG, "n must be a multiple of groups%s");
  if (out_z && !z) return fail(CMCD_ERR_BAD_ARG, "out_z needs z%s");
  if (z && dim < 1) return fail(CMCD_ERR_BAD_ARG, "dim must be >= 1%s");
  if (n / groups > kResampleMaxGroup)
    return fail(CMCD_ERR_UNSUPPORTED, "groups of more than 2^20 particles are not resampled (got %s%lld)", "", n / groups);
  int rc = check_workspace(workspace, workspace_bytes, resample_workspace_bytes(n));
  if (rc != CMCD_OK) return rc;
  return resample_launch(loss, z, n, dim, groups, seed, workspace, out_index, out_z, out_stats,
                         static_cast<hipStream_t>(stream_));
}

// the shape checks the three cmcd_sinkhorn_* calls share; 0 = fine
static int check_sinkhorn_shape(int64_t n, int32_t dim, int32_t groups) {
  if (n < 2) return fail(CMCD_ERR_BAD_ARG, "n must be >= 2%s");
  if (dim < 1) return fail(CMCD_ERR_BAD_ARG, "dim must be >= 1%s");
  if (groups < 1) return fail(CMCD_ERR_BAD_ARG, "groups must be >= 1%s");
  if (n > kSinkhornMaxN)
    return fail(CMCD_ERR_UNSUPPORTED, "clouds of more than 8192 points are not solved (got %s%lld)", "", n);
  if (groups > kSinkhornMaxGroups)
    return fail(CMCD_ERR_UNSUPPORTED, "more than 65535 problems per call are not solved (got %s%lld)", "", groups);
  return CMCD_OK;
}

int64_t cmcd_sinkhorn_workspace_bytes(int64_t n, int32_t dim, int32_t groups) {
  if (n < 2 || n > kSinkhornMaxN || dim < 1 || groups < 1 || groups > kSinkhornMaxGroups) return 0;
  return sinkhorn_workspace_bytes(n, groups);
}

int cmcd_sinkhorn_setup(const double* x, const double* y, const double* a, const double* b, int64_t n, int32_t dim,
                        int32_t groups, double reg, void* workspace, int64_t workspace_bytes, void* stream_) {
  if (!x || !y) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  int rc = check_sinkhorn_shape(n, dim, groups);
  if (rc != CMCD_OK) return rc;
  if (!(reg > 0.0) || reg > 1.79769313486231570815e308) return fail(CMCD_ERR_BAD_ARG, "reg must be positive and finite%s");
  if ((rc = check_workspace(workspace, workspace_bytes, sinkhorn_workspace_bytes(n, groups))) != CMCD_OK) return rc;
  return sinkhorn_setup_launch(x, y, a, b, n, dim, groups, reg, workspace, static_cast<hipStream_t>(stream_));
}

int cmcd_sinkhorn_iterate(int64_t n, int32_t dim, int32_t groups, int32_t first_iteration, int32_t count,
                          int32_t num_iter_max, double stop_thr, void* workspace, int64_t workspace_bytes,
                          int32_t* done_flags, void* stream_) {
  int rc = check_sinkhorn_shape(n, dim, groups);
  if (rc != CMCD_OK) return rc;
  if (num_iter_max < 1 || num_iter_max == INT32_MAX) return fail(CMCD_ERR_BAD_ARG, "num_iter_max out of range%s");
  if (first_iteration < 0 || count < 0 || count > num_iter_max - first_iteration)
    return fail(CMCD_ERR_BAD_ARG, "iterations must lie in [0, num_iter_max]%s");
  if ((rc = check_workspace(workspace, workspace_bytes, sinkhorn_workspace_bytes(n, groups))) != CMCD_OK) return rc;
  return sinkhorn_iterate_launch(n, groups, first_iteration, count, num_iter_max, stop_thr, workspace, done_flags,
                                 static_cast<hipStream_t>(stream_));
}

int cmcd_sinkhorn_cost(const double* x, const double* y, int64_t n, int32_t dim, int32_t groups, void* workspace,
                       int64_t workspace_bytes, double* out, int32_t* done_flags, void* stream_) {
  if (!x || !y || !out) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  int rc = check_sinkhorn_shape(n, dim, groups);
  if (rc != CMCD_OK) return rc;
  if ((rc = check_workspace(workspace, workspace_bytes, sinkhorn_workspace_bytes(n, groups))) != CMCD_OK) return rc;
  return sinkhorn_cost_launch(x, y, n, dim, groups, workspace, out, done_flags, static_cast<hipStream_t>(stream_));
}

#ifndef CMCD_NO_DIAG_HOOKS   // include/cmcd_hip_diag.h: compiled out of a boundary-only build
const char* cmcd_last_kernel_name(void) { return g_kernel_name; }

int cmcd_debug_capture_noise(uint32_t* bits, uint32_t* gen_keys, float* noise) {
  if ((bits == nullptr) != (noise == nullptr)) return fail(CMCD_ERR_BAD_ARG, "bits and noise go together%s");
  g_capture.bits = bits; g_capture.keys = gen_keys; g_capture.noise = noise;
  return CMCD_OK;
}

int cmcd_debug_grad_item(int mode) {
  if (mode < -1 || mode > 1) return fail(CMCD_ERR_BAD_ARG, "mode must be -1, 0 or 1%s");
  set_grad_item_override(mode);
  return CMCD_OK;
}

int cmcd_profile_enable(int on) {
  g_prof.on = on != 0;
  g_prof.used = 0;
  // the first 512 event pairs are created here, outside any timed region (a 20-step measurement would otherwise pay two
  // hipEventCreate calls inside every one of its steps)
  for (; on && g_prof.created < 512; ++g_prof.created) {
    CMCD_HIP_CHECK(hipEventCreate(&g_prof.ev[g_prof.created][0]));
    CMCD_HIP_CHECK(hipEventCreate(&g_prof.ev[g_prof.created][1]));
  }
  return CMCD_OK;
}

int cmcd_profile_collect(double* total_ms, int64_t* launches) {
  if (!total_ms || !launches) return fail(CMCD_ERR_BAD_ARG, "null pointer argument%s");
  double tot = 0.0;
  for (int i = 0; i < g_prof.used; ++i) {
    float ms = 0.f;
    CMCD_HIP_CHECK(hipEventSynchronize(g_prof.ev[i][1]));
    CMCD_HIP_CHECK(hipEventElapsedTime(&ms, g_prof.ev[i][0], g_prof.ev[i][1]));
    tot += ms;
  }
  *total_ms = tot;
  *launches = g_prof.used;
  g_prof.used = 0;
  return CMCD_OK;
}
#endif   // CMCD_NO_DIAG_HOOKS

}  // extern "C"
