// Host-side seams between cmcd_api.hip (the C ABI: validation, workspace plan, kernel selection) and cmcd_kernels.hip (the prep,
// trajectory and merge kernels with their launchers), cmcd_reverse[_uha].hip, cmcd_segment[_uha].hip, cmcd_resample.hip and cmcd_sinkhorn.hip,
// plus the two host helpers every entry point shares (al4, check_many_gmm).  cmcd_reverse[_uha].hip, cmcd_segment[_uha].hip, cmcd_grad.hip,
// cmcd_mfvi.hip and cmcd_hais.hip include it through cmcd_tile.h, which holds the wave-per-tile pieces they share.  The seams of
// the translation units that do not include it (the coop, lgcp, uha, bptt and opt files) are in cmcd_common.h, which the stored
// counter figures are hashed over (bench.py: kernel_sources_sha).
#pragma once
#include <hip/hip_runtime.h>

#include "cmcd_common.h"

namespace cmcd {

// cmcd_api.hip: sets this host thread's cmcd_last_error and returns `code`
int fail(int code, const char* fmt, const char* a = "", long long b = 0);

#define CMCD_HIP_CHECK(expr)                                                                   \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(CMCD_ERR_HIP, "HIP error: %s (code %lld)", hipGetErrorString(e_), (long long)e_); \
  } while (0)

// workspace blocks start on 16 bytes: a float count rounded up to a multiple of four
inline int64_t al4(int64_t x) { return (x + 3) & ~int64_t(3); }

// many_gmm takes target_consts = {scale, means[n_mixes][2]} with at most 64 mixtures (the block the kernels stage into LDS); any
// other target: nothing to check here.  n_mix (nullable) receives the number of mixtures, 0 for another target.
inline int check_many_gmm(int target, const float* target_consts, int64_t n_target, int* n_mix = nullptr) {
  if (n_mix) *n_mix = 0;
  if (target != CMCD_TARGET_MANY_GMM) return CMCD_OK;
  if (!target_consts || n_target < 3 || (n_target - 1) % 2 != 0 || (n_target - 1) / 2 > 64)
    return fail(CMCD_ERR_BAD_ARG, "many_gmm needs target_consts = {scale, means[n_mixes<=64][2]}%s");
  if (n_mix) *n_mix = int((n_target - 1) / 2);
  return CMCD_OK;
}

// cmcd_kernels.hip.  The launchers that return void leave their launch status to the caller's hipGetLastError.
// `d` is the effective descriptor of the call (cmcd_api.hip: CallPlan).
bool traj_available(const cmcd_desc& d, int T);   // a wave-per-tile traj_kernel instance exists for (target, dim, arch, T)
// before_launch: called once the checks have passed, right in front of the kernel launch (the profile's start event); non-zero = give up
int traj_launch(const cmcd_desc& d, const WsLayout& w, const TrajArgs& ta, hipStream_t stream,
                int (*before_launch)(hipStream_t) = nullptr);
// schedule tables + first-layer bias table + packed weights, one launch; stamp: tables_stamp() of the forming call
void launch_prep(const cmcd_desc& d, const cmcd_layout& lay, const WsLayout& w, const float* params,
                 const float* target_consts, int n_mix, float* ws, hipStream_t stream, uint32_t stamp);
// the schedule tables alone (lgcp: the rest of its tables belongs to cmcd_lgcp.hip)
void launch_prep_sched(const cmcd_desc& d, const cmcd_layout& lay, const WsLayout& w, const float* params, float* ws,
                       hipStream_t stream, uint32_t stamp);
// fixed-order merge of `count` statistics records -> out5; stamp_slot non-null: NaN unless *stamp_slot == stamp (prepared
// form).  cmcd_common.h's four-argument launch_finalize (cmcd_mfvi.hip's call) is this one without a stamp.
void launch_finalize(const double* partials, int32_t count, double* out5, hipStream_t stream, const uint32_t* stamp_slot,
                     uint32_t stamp);
void launch_vargrad_weights(const float* loss, const double* stats, int64_t n, int64_t n_total, float* omega,
                            hipStream_t stream);

// cmcd_reverse.hip: the reverse-time chain of the overdamped modes (target draws x[n][dim] through the backward kernels), one
// wave per 16-particle tile.  Reads the tables launch_prep left in ta.ws; ta.out_loss receives w, ta.out_z the end state z_0,
// ta.partials one statistics record per tile (w.n_waves of them) over l := w.  No instance for MCD_CAIS_UHA_sn and lgcp.
bool reverse_available(const cmcd_desc& d, int T);
int reverse_launch(const cmcd_desc& d, const WsLayout& w, const TrajArgs& ta, const float* x, hipStream_t stream);

// cmcd_segment.hip: bridges [k0, k1) of the overdamped forward chain from a caller-supplied state (z, wpath, key), one wave per
// 16-particle tile.  Reads the tables launch_prep left in ta.ws and ta.seeds when k0 == 0; z / wpath / key are read (k0 > 0) and
// overwritten in place, lg receives log gamma_k1(z), ta.partials one statistics record per tile over l := -(wpath + lg).
// The instances of the reverse call; none for MCD_CAIS_UHA_sn and lgcp.
bool segment_available(const cmcd_desc& d, int T);
int segment_launch(const cmcd_desc& d, const WsLayout& w, const TrajArgs& ta, int32_t k0, int32_t k1, float* z, float* wpath,
                   uint32_t* key, float* lg, hipStream_t stream);

// cmcd_segment_uha.hip: the same for MCD_CAIS_UHA_sn, whose particle state carries the momentum: bridges [k0, k1) of the 2nd-order
// forward chain from (z, rho, wpath, key), one wave per 16-particle tile.  lg receives log gamma_k1(z) + log N(rho; 0, I).  The
// instances of uha_traj_kernel (dds 64; geffner on 2 / 4 / 5 / 9 neuron tiles); none for the other modes and lgcp.  Its launch
// sizes LDS for a first layer with 2 dim input rows, with tile_launch's waves-per-workgroup rule.
bool segment_uha_available(const cmcd_desc& d, int T);
int segment_uha_launch(const cmcd_desc& d, const WsLayout& w, const TrajArgs& ta, int32_t k0, int32_t k1, float* z, float* rho,
                       float* wpath, uint32_t* key, float* lg, hipStream_t stream);

// cmcd_reverse_uha.hip: the reverse-time chain of MCD_CAIS_UHA_sn (target draws x[n][dim] through the backward momentum kernels and
// the inverted leap-frogs), one wave per 16-particle tile.  ta.out_loss receives w, ta.out_z the end state z_0, rho0 the end
// momentum, ta.partials one statistics record per tile over l := w.  The instances and the launch rule of segment_uha_launch; none
// for the other modes and lgcp.
bool reverse_uha_available(const cmcd_desc& d, int T);
int reverse_uha_launch(const cmcd_desc& d, const WsLayout& w, const TrajArgs& ta, const float* x, float* rho0,
                       hipStream_t stream);

// cmcd_ldvi.hip: LDVI (MCD_U_a-lp-sn / MCD_U_a-lp, include/cmcd_hip.h: cmcd_ldvi_bound_grad), one wave per 16-particle tile.
// `d` is the effective descriptor whose tables launch_prep left in ws (use_net: CMCD_MODE_CAIS_UHA_SN on the geffner net;
// otherwise CMCD_MODE_ULA: schedule tables and target constants only).  The forward chain leaves one statistics record per tile
// at ws + w.partials; with `grad` non-null it keeps its states in gws (ldvi_grad_floats floats) and the gradient launches follow.
bool ldvi_available(const cmcd_desc& d, int T, bool use_net);
int64_t ldvi_grad_floats(const cmcd_desc& d, int HP, int64_t n, bool use_net);
int ldvi_launch(const cmcd_desc& d, const cmcd_layout& lay, const WsLayout& w, bool use_net, const int32_t* seeds, int64_t n,
                const float* params, int64_t n_params, float* ws, float* gws, float omega, float* out_loss, float* out_z,
                float* grad, hipStream_t stream);

// cmcd_reverse_ldvi.hip: the reverse-time chain of LDVI (include/cmcd_hip.h: cmcd_bound_reverse_ldvi), one wave per 16-particle
// tile.  `d`, `w` and the tables in ws as for ldvi_launch; out_w receives w, out_z0 / out_rho0 the state at the q end, ws +
// w.partials one statistics record per tile over l := w.  The instances and the launch rule of ldvi_traj_kernel.
bool reverse_ldvi_available(const cmcd_desc& d, int T, bool use_net);
int reverse_ldvi_launch(const cmcd_desc& d, const cmcd_layout& lay, const WsLayout& w, bool use_net, const int32_t* seeds,
                        const float* x, int64_t n, const float* params, float* ws, float* out_w, float* out_z0, float* out_rho0,
                        hipStream_t stream);

// cmcd_reverse_hais.hip: the reverse-time chain of UHA (include/cmcd_hip.h: cmcd_bound_reverse_hais), the mapping, instances and
// shape limits of hais_traj_kernel.  The workspace holds one statistics record per 16-particle tile (reverse_hais_floats floats);
// the arguments of the launch are the entry point's, already checked.
bool reverse_hais_available(int target, int dim);
bool reverse_hais_shape_ok(int32_t nbridges, int32_t lfsteps, int64_t n);
int64_t reverse_hais_floats(int64_t n);
int reverse_hais_launch(int target, int dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout& lay, const int32_t* seeds,
                        const float* x, int64_t n, const float* params, const float* target_consts, int n_mix, float* ws,
                        float* out_w, float* out_z0, float* out_rho0, hipStream_t stream);

// cmcd_segment_ldvi.hip: bridges [k0, k1) of the LDVI forward chain from (z, rho, wpath, key) (include/cmcd_hip.h:
// cmcd_bound_segment_ldvi), one wave per 16-particle tile.  `d`, `w` and the tables in ws as for ldvi_launch; seeds are read when
// k0 == 0; z / rho / wpath / key are read (k0 > 0) and overwritten in place, lg receives log gamma_k1(z) + log N(rho; 0, I), ws +
// w.partials one statistics record per tile over l := -(wpath + lg).  The instances and the launch rule of ldvi_traj_kernel.
bool segment_ldvi_available(const cmcd_desc& d, int T, bool use_net);
int segment_ldvi_launch(const cmcd_desc& d, const cmcd_layout& lay, const WsLayout& w, bool use_net, int32_t k0, int32_t k1,
                        const int32_t* seeds, int64_t n, const float* params, float* ws, float* z, float* rho, float* wpath,
                        uint32_t* key, float* lg, hipStream_t stream);

// cmcd_segment_hais.hip: the same for UHA (include/cmcd_hip.h: cmcd_bound_segment_hais); rho is the momentum between bridges and lg
// = log gamma_k1(z) alone.  The mapping and instances of hais_traj_kernel, the shape limits and the workspace of the reverse call
// (reverse_hais_shape_ok, reverse_hais_floats: one statistics record per tile); the arguments are the entry point's, already checked.
bool segment_hais_available(int target, int dim);
int segment_hais_launch(int target, int dim, int32_t nbridges, int32_t lfsteps, const cmcd_hais_layout& lay, int32_t k0, int32_t k1,
                        const int32_t* seeds, int64_t n, const float* params, const float* target_consts, int n_mix, float* ws,
                        float* z, float* rho, float* wpath, uint32_t* key, float* lg, hipStream_t stream);

// cmcd_resample.hip: importance statistics + systematic resampling, one workgroup per group of n / groups rows, one launch.
// The group is walked in chunks of kResampleChunk rows with a float64 running sum carried between them.
constexpr int kResampleChunk = 1024;
constexpr int64_t kResampleMaxGroup = int64_t(1) << 20;   // rows per group the entry point accepts
int64_t resample_workspace_bytes(int64_t n);
// the arguments are cmcd_resample_systematic's, already checked; out_index / out_z / z nullable
int resample_launch(const float* loss, const float* z, int64_t n, int32_t dim, int32_t groups, uint32_t seed, void* workspace,
                    int32_t* out_index, float* out_z, double* out_stats, hipStream_t stream);

// cmcd_sinkhorn.hip: batched float64 Sinkhorn between equal-size clouds, grid (row tiles, problems), one launch per iteration.
constexpr int kSinkhornRows = 64;          // rows of K per workgroup
constexpr int kSinkhornThreads = 256;
constexpr int64_t kSinkhornMaxN = 8192;    // v[n] stays in LDS: 64 KiB of doubles
constexpr int32_t kSinkhornMaxGroups = 65535;   // gridDim.y
int64_t sinkhorn_workspace_bytes(int64_t n, int32_t groups);
// the arguments are those of the cmcd_sinkhorn_* entry points, already checked; a / b / done_flags nullable
int sinkhorn_setup_launch(const double* x, const double* y, const double* a, const double* b, int64_t n, int32_t dim,
                          int32_t groups, double reg, void* workspace, hipStream_t stream);
int sinkhorn_iterate_launch(int64_t n, int32_t groups, int32_t first_iteration, int32_t count, int32_t num_iter_max,
                            double stop_thr, void* workspace, int32_t* done_flags, hipStream_t stream);
int sinkhorn_cost_launch(const double* x, const double* y, int64_t n, int32_t dim, int32_t groups, void* workspace, double* out,
                         int32_t* done_flags, hipStream_t stream);

}  // namespace cmcd
