// C ABI of libneuray_hip.so (declared in include/neuray_hip.h).  Host-side launch logic only; the device
// code lives in nr_kernels.h / nr_device.h.  Built with hipcc --offload-arch=gfx950 (product) or, for the
// CPU test emulator, g++ -DNEURAY_EMU (tests/emu/build_emu.py).
#include "nr_kernels.h"
#include "nr_kernels_bwd.h"
#include "nr_kernels_norm.h"
#include "nr_kernels_conv3d.h"
#include "nr_kernels_conv2d.h"
#include "nr_kernels_metrics.h"
#include "nr_kernels_loss.h"
#include "nr_kernels_lpips.h"
#include "nr_kernels_proc.h"
// the plain bf16-operand build is inference only; the fp32 build and the split build (hi + lo bf16 operands: fp32-grade products)
// carry the training path
#if defined(NR_BF16_QUADS) && !defined(NR_BF16_SPLIT)
#define NR_INFERENCE_ONLY 1
#else
#include "nr_kernels_bwd2.h"
#endif
#include "nr_kernels_dr.h"          // (after the NR_INFERENCE_ONLY decision: its backward half is training only)
#ifndef NR_BF16_QUADS
#include "nr_kernels_vis.h"         // (fp32 MFMA only: the bf16-operand builds leave the visibility entries returning an error)
#include "nr_kernels_fuse.h"        // (the fp32 library only, like the visibility entries)
#include "nr_kernels_tsdf.h"        // (likewise)
#include "nr_kernels_aug.h"         // (likewise)
#include "nr_kernels_stereo.h"      // (likewise)
#endif
#include "nr_pack.h"
#include "../../include/neuray_hip.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>

namespace {

thread_local char g_err[512] = "";

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: %s", what, hipGetErrorString(e));
    return 0;
}

int grid_for(long long work_items, int per_block, int max_blocks) {
    long long b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int)b;
}

// Kernels with dynamic LDS.  A kernel may use more than 64 KB only after its limit was raised; that call costs host time on every launch,
// so launch_lds makes it past 64 KB only, or - `always` - where a site's kernel is known to be above it.  The kernel arrives as a function
// pointer: the emulator's NR_LAUNCH calls it inside a [=] lambda.
template <class K>
void allow_lds(K k, size_t smem) {
#ifndef NEURAY_EMU
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
#else
    (void)k; (void)smem;
#endif
}
template <class K, class P>
void launch_lds(K k, dim3 grid, dim3 block, size_t smem, void* stream, const P& p, bool always = false) {
    if (always || smem > 64 * 1024) allow_lds(k, smem);
    NR_LAUNCH(k, grid, block, smem, stream, p);
}

static_assert(NEURAY_POINT_REC == nr::kPointRec, "abi");
static_assert(NEURAY_VIEW_CONST == nr::kViewConst, "abi");
static_assert(NEURAY_QUERY_CONST == nr::kQueryConst, "abi");
static_assert(NEURAY_PASS_TENSORS == nr::T_COUNT, "abi");
static_assert(NEURAY_DBG_FIELDS == nr::kDbgFields, "abi");
static_assert(NEURAY_RAY_ATT_SAVE == nr::kRayAttSave, "abi");
static_assert(NEURAY_MAX_SAMPLES == nr::kMaxSamples, "abi");
#ifndef NR_BF16_QUADS
static_assert(NEURAY_FUSE_MAX_SRC == nr::kFuseMaxSrc, "abi");
#endif
static_assert(NEURAY_PROC_HEADER == nr::kProcHeader && NEURAY_PROC_PRIM == nr::kProcPrim && NEURAY_PROC_MAX_PRIMS == nr::kProcMaxPrims, "abi");

template <int NT, int VPW, bool HAS_VIS, int OWN, int MINW, bool SAVE, int AR, bool ONEB>
int launch_points_form(const nr::PointParams& p, void* stream) {
    const int npts = p.rn * p.dn;
    const int nwaves = (p.rfn + VPW - 1) / VPW;
    const size_t smem = nr::point_smem_bytes<NT>(nwaves, AR, ONEB);
    if (smem > 160 * 1024) return fail("neuray_render_points: %zu bytes of LDS needed (rfn=%d)", smem, p.rfn);
    // persistent-style grid: enough workgroups to fill the 768 resident slots (3 per CU) twenty times over, grid-stride beyond.  Measured on
    // the 800 x 800 workload (131 072 tiles per coarse launch), same box: 768 workgroups 2.30 M rays/s, 1536 2.35, 3072 / 3840 2.38,
    // 4096 2.42, 6144 2.37, 8192 ... 32768 2.44 - finer-grained balancing wins over fewer prologues, and counts that divide the tiles
    // evenly beat those that do not.  Round 4 (tiles of 16 neighbouring rays): 4096 5.59 ms per launch, 8192 5.49, 16384 5.47, 32768 5.55.
#ifndef NR_POINT_GRID
#define NR_POINT_GRID (256 * 64)
#endif
    int grid = grid_for(npts, 16 * NT, NR_POINT_GRID);
#ifndef NR_POINT_MIN_TILES
#define NR_POINT_MIN_TILES 2       // a workgroup's prologue (constants, first weight phase) wants at least this many tiles behind it
#endif
    if (!SAVE && npts / 16 >= 4096 && grid > npts / (16 * NR_POINT_MIN_TILES)) grid = npts / (16 * NR_POINT_MIN_TILES);
    grid = (grid + 7) / 8 * 8;                         // the XCD-aware tile map needs a multiple of 8
    const int threads = 64 * nwaves;
    // __launch_bounds__(1024) caps the kernel at 128 VGPRs so that 4 waves share a SIMD (DESIGN.md "occupancy")
    auto k = nr::points_kernel<NT, VPW, HAS_VIS, OWN, 1024 / VPW, MINW, SAVE, false, AR, ONEB>;
    if constexpr (!SAVE) {
        if (p.dbg) k = nr::points_kernel<NT, VPW, HAS_VIS, OWN, 1024 / VPW, MINW, false, true, AR, ONEB>;     // the per-view record: its own instantiation
    } else if (p.dbg) {
        return fail("neuray_render_points: dbg_dev and saved_dev together are not built (run the pass twice)");
    }
    launch_lds(k, dim3(grid), dim3(threads), smem, stream, p);
    return check_launch("neuray_render_points");
}

// The form of the cross-view all-reduces (nr_device.h): one barrier where the two banks fit (nr::point_one_barrier: the AR_X3 kernel up to
// six waves), two barriers elsewhere.  NEURAY_POINT_ALLREDUCE=2 forces the two-barrier form from the same library (A/B hook of
// tools/ab_forward.py and tests/test_allreduce_forms.py, read at every launch so that one process can run both); the results are
// bit-identical.
template <int NT, int VPW, bool HAS_VIS, int OWN, int MINW, bool SAVE = false, int AR = nr::AR_F32>
int launch_points_own(const nr::PointParams& p, void* stream) {
    if constexpr (AR == nr::AR_X3) {
        const char* e = getenv("NEURAY_POINT_ALLREDUCE");
        if (!(e && atoi(e) == 2) && nr::point_one_barrier<NT>((p.rfn + VPW - 1) / VPW, AR))
            return launch_points_form<NT, VPW, HAS_VIS, OWN, MINW, SAVE, AR, true>(p, stream);
    }
    return launch_points_form<NT, VPW, HAS_VIS, OWN, MINW, SAVE, AR, false>(p, stream);
}

template <int NT, int VPW, bool HAS_VIS, int MINW, int AR = nr::AR_F32>
int launch_points(const nr::PointParams& p, void* stream) {
    const int nwaves = (p.rfn + VPW - 1) / VPW;
    if (nwaves >= 4) return launch_points_own<NT, VPW, HAS_VIS, 1, MINW, false, AR>(p, stream);
    if (nwaves >= 2) return launch_points_own<NT, VPW, HAS_VIS, 2, MINW, false, AR>(p, stream);
    return launch_points_own<NT, VPW, HAS_VIS, 4, MINW, false, AR>(p, stream);
}

// training forward: the same kernels with the cross-view quantities written out for the resident backward (rfn <= 8; two views per
// wave, one for a single view)
template <bool HAS_VIS>
int launch_points_save(const nr::PointParams& p, void* stream) {
#ifdef NR_INFERENCE_ONLY
    return fail("neuray_render_points: saved_dev is a training feature; the bf16-operand variant is inference only");
#else
    if (p.rfn > 8) return fail("neuray_render_points: saved_dev needs rfn <= 8 (rfn=%d)", p.rfn);
    if (p.rfn == 1) return launch_points_own<1, 1, HAS_VIS, 4, 4, true>(p, stream);
    const int nwaves = (p.rfn + 1) / 2;
    if (nwaves >= 4) return launch_points_own<1, 2, HAS_VIS, 1, 3, true>(p, stream);
    if (nwaves >= 2) return launch_points_own<1, 2, HAS_VIS, 2, 3, true>(p, stream);
    return launch_points_own<1, 2, HAS_VIS, 4, 3, true>(p, stream);
#endif
}

// Built decompositions (measured on MI355X, DESIGN.md "point kernel tuning"):
//   views_per_wave = 2, 168 VGPRs, 3 waves per SIMD  - default (2.35 M rays/s on the lego-800 workload)
//   views_per_wave = 1, 128 VGPRs, 4 waves per SIMD  - single reference view, and the A/B reference
#ifndef NR_POINT_MINW
#define NR_POINT_MINW 3        // workgroups per CU the 2-views-per-wave kernel is compiled for (A/B: -DNR_POINT_MINW=2 = 256 VGPRs, no spills)
#endif
#ifndef NR_POINT_MINW_X3
#define NR_POINT_MINW_X3 2     // the same for the AR_X3 instantiation: 207 VGPRs, no spills; compiled for 3 (168 VGPRs, 33 spilled) it is 8.5 % slower (profiles/r06_c_*)
#endif
template <bool HAS_VIS>
int launch_points_cfg(const nr::PointParams& p, int vpw, int arith, void* stream) {
    if (arith == NEURAY_ARITH_X3) {
#ifdef NR_BF16_QUADS
        return fail("neuray_render_points: arith = NEURAY_ARITH_X3 lives in the fp32 library (this is a bf16-operand variant build)");
#else
        if (vpw == 2) return launch_points<1, 2, HAS_VIS, NR_POINT_MINW_X3, nr::AR_X3>(p, stream);
        return fail("neuray_render_points: arith = NEURAY_ARITH_X3 is built for views_per_wave = 2 (rfn >= 2)");
#endif
    }
    if (vpw == 2) return launch_points<1, 2, HAS_VIS, NR_POINT_MINW>(p, stream);
    if (vpw == 1) return launch_points<1, 1, HAS_VIS, 4>(p, stream);
    return fail("neuray_render_points: views_per_wave=%d is not built (1 or 2)", vpw);
}

}  // namespace

namespace {
template <int NT, int MTW, int WC = 1, bool RELU = false>
void launch_conv2d_x3(const nr::Conv2dX3Params& p, int bands, void* stream) {
    const int lw = p.tw + 2, hp = p.h + 2 * p.pad;
    const long long q = (long long)p.n * hp * lw;
    const int per = nr::kC2Waves * NT * 16;
    const size_t smem = (size_t)nr::conv2d_x3_smem_bytes(NT, lw);
    launch_lds(nr::conv2d_x3_kernel<NT, MTW, WC, RELU>, dim3((unsigned)((q + per - 1) / per), (unsigned)(p.cout / 16 / MTW / WC), (unsigned)bands),
               dim3(64 * nr::kC2Waves * WC), smem, stream, p);
}
int g_conv2d_nt = 0, g_conv2d_mtw = 0;     // NEURAY_CONV2D_NT / _MTW: tile-shape overrides (set by hand; see conv3x3_x3_impl)
}  // namespace

extern "C" {

int neuray_abi_version(void) { return NEURAY_ABI_VERSION; }
const char* neuray_last_error(void) { return g_err; }
int neuray_is_device_build(void) {
#ifdef NEURAY_EMU
    return 0;
#else
    return 1;
#endif
}

size_t neuray_packed_pass_floats(void) { return (size_t)nr::kPackedPassFloats; }

int neuray_pack_pass_weights(const float* const* tensors_host, float* packed_host) {
    if (!tensors_host || !packed_host) return fail("neuray_pack_pass_weights: null argument");
    const int rc = nr::pack_pass_weights(tensors_host, packed_host);
    if (rc) return fail("neuray_pack_pass_weights: tensor %d of the pass is missing", rc - 1);
    return 0;
}

int neuray_pack_pass_weights_folded(const float* const* tensors_host, float* packed_host) {
    if (!tensors_host || !packed_host) return fail("neuray_pack_pass_weights_folded: null argument");
    const int rc = nr::pack_pass_weights(tensors_host, packed_host, true);
    if (rc) return fail("neuray_pack_pass_weights_folded: tensor %d of the pass is missing", rc - 1);
    return 0;
}

size_t neuray_packed_points_floats_x3(void) { return (size_t)nr::kPackedPointFloatsX3; }

int neuray_pack_pass_weights_x3(const float* const* tensors_host, float* packed_host) {
    if (!tensors_host || !packed_host) return fail("neuray_pack_pass_weights_x3: null argument");
    const int rc = nr::pack_pass_weights_x3(tensors_host, packed_host);
    if (rc) return fail("neuray_pack_pass_weights_x3: tensor %d of the pass is missing", rc - 1);
    return 0;
}

int neuray_mt19937_shuffle(unsigned int* key624_host, int* pos_host, void* data_host, long long n, int itemsize) {
    if (nr::mt19937_shuffle(key624_host, pos_host, data_host, n, itemsize))
        return fail("neuray_mt19937_shuffle: needs key[624], 0 <= pos <= 624, a data pointer and 4- or 8-byte items");
    return 0;
}

int neuray_operand_precision(void) {
#if defined(NR_BF16_SPLIT)
    return 48;         // hi + lo bf16 operands, three bf16 MFMAs per fp32 quad (libneuray_hip_bf16x3.so)
#elif defined(NR_BF16_QUADS)
    return 16;
#else
    return 32;
#endif
}

int neuray_pack_pass_index_map(int has_vis_head, int* index_host, float* scale_host) {
    if (!index_host || !scale_host) return fail("neuray_pack_pass_index_map: null argument");
#ifdef NR_INFERENCE_ONLY
    return fail("neuray_pack_pass_index_map: the bf16-operand build packs on the host only (inference variant, no training path)");
#endif
    if (nr::pack_pass_index_map(has_vis_head != 0, index_host, scale_host)) return fail("neuray_pack_pass_index_map: internal error");
    return 0;
}

// float ranges [begin, end) of the quad fragments inside the packed pass buffer (transposed = 0) or the transposed pack (= 1): what a
// device-side packer of the split library converts from four fp32 weights to (hi pair, hi pair, lo pair, lo pair) after the gather
int neuray_packed_quad_ranges(int transposed, int* ranges_host, int max_pairs) {
    if (!ranges_host || max_pairs < 1) return fail("neuray_packed_quad_ranges: null argument");
    int n = 0;
    const int first = transposed ? (int)nr::L_FWD_COUNT : 0, last = transposed ? (int)nr::L_COUNT : (int)nr::L_FWD_COUNT;
    for (int l = first; l < last; ++l) {
        if (nr::quads_floats(l) == 0) continue;
        if (n >= max_pairs) return fail("neuray_packed_quad_ranges: more than %d ranges", max_pairs);
        ranges_host[2 * n] = nr::quads_offset(l);
        ranges_host[2 * n + 1] = nr::quads_offset(l) + nr::quads_floats(l);
        ++n;
    }
    return -n;          // (negative count on success: 0 is reserved for "no error" elsewhere, positive for failure)
}

int neuray_setup_views(const float* poses, const float* Ks, const float* depth_range, int n, float* out, void* stream) {
    if (n < 1 || n > NEURAY_MAX_VIEWS) return fail("neuray_setup_views: n=%d outside [1,%d]", n, NEURAY_MAX_VIEWS);
    NR_LAUNCH(nr::view_setup_kernel, dim3(1), dim3(64), 0, stream, poses, Ks, depth_range, n, out);
    return check_launch("neuray_setup_views");
}

int neuray_setup_query(const float* pose, const float* Kinv, const float* depth_range, float* out, void* stream) {
    NR_LAUNCH(nr::query_setup_kernel, dim3(1), dim3(64), 0, stream, pose, Kinv, depth_range, out);
    return check_launch("neuray_setup_query");
}

int neuray_relayout_nhwc(const float* src, float* dst, int n, int c, int h, int w, int c_pad, void* stream) {
    if (c_pad < c || n < 1) return fail("neuray_relayout_nhwc: bad shape n=%d c=%d c_pad=%d", n, c, c_pad);
    const int grid = grid_for((long long)n * h * w, 256, 256 * 16);
    NR_LAUNCH(nr::relayout_kernel, dim3(grid), dim3(256), 0, stream, src, dst, n, c, h, w, c_pad);
    return check_launch("neuray_relayout_nhwc");
}

int neuray_sample_coarse_depth(const float* depth_range, int rn, int dn, float* depth, void* stream) {
    return neuray_sample_coarse_depth_jittered(depth_range, nullptr, rn, dn, depth, stream);
}

int neuray_sample_coarse_depth_jittered(const float* depth_range, const float* uniforms, int rn, int dn, float* depth, void* stream) {
    if (dn <= 2) return fail("neuray_sample_coarse_depth: dn=%d must be > 2 (render_ops.py:157)", dn);
    const int grid = grid_for((long long)rn * dn, 256, 256 * 8);
    NR_LAUNCH(nr::coarse_depth_kernel, dim3(grid), dim3(256), 0, stream, depth_range, uniforms, rn, dn, depth);
    return check_launch("neuray_sample_coarse_depth");
}

int neuray_render_points(const NeurayPointsArgs* a, void* stream) {
    if (!a) return fail("neuray_render_points: null args");
    if (a->rfn < 1 || a->rfn > NEURAY_MAX_VIEWS) return fail("neuray_render_points: rfn=%d outside [1,%d]", a->rfn, NEURAY_MAX_VIEWS);
    if (a->dn <= 2 || a->rn < 1) return fail("neuray_render_points: bad rn=%d dn=%d", a->rn, a->dn);
    if (a->use_vis && !a->has_vis_head) return fail("neuray_render_points: use_vis set but the decoder has no vis head");
    if ((long long)a->rn * a->dn > 0x7fffffffLL / 2) return fail("neuray_render_points: rn*dn too large for one call");
    nr::PointParams p;
    p.que_const = a->query_const_dev; p.view_const = a->view_const_dev; p.coords = a->coords_dev; p.depth = a->depth_dev;
    p.ray_feats = a->ray_feats_nhwc_dev; p.img_feats = a->img_feats_nhwc_dev; p.rgba = a->rgba_dev;
    p.weights = a->packed_weights_dev; p.point_out = a->point_out_dev; p.dbg = a->dbg_dev; p.saved = a->saved_dev;
    p.rfn = a->rfn; p.rn = a->rn; p.dn = a->dn; p.h = a->h; p.w = a->w; p.fh = a->fh; p.fw = a->fw;
    p.use_vis = a->use_vis; p.var_bias = a->var_bias; p.folded = a->folded; p.slot_stats = a->slot_stats_dev;
    if (a->folded && a->saved_dev) return fail("neuray_render_points: saved_dev (training forward) takes the unfolded pack");
    if (a->arith != NEURAY_ARITH_F32 && a->arith != NEURAY_ARITH_X3) return fail("neuray_render_points: arith=%d is not built (0 or 1)", a->arith);
    if (a->arith == NEURAY_ARITH_X3 && a->saved_dev) return fail("neuray_render_points: saved_dev (training forward) runs on NEURAY_ARITH_F32");
    // work decomposition: reference views processed per wave (0 = default)
    int vpw = a->views_per_wave ? a->views_per_wave : (a->rfn >= 2 ? 2 : 1);
    // the vis head is only evaluated when compute_prob consumes it (a fine decoder's vis head is ignored on the
    // reference-view path when the coarse decoder has use_vis = False: quirk A.9.2)
    const bool vis = a->has_vis_head && a->use_vis;
    if (a->saved_dev) return vis ? launch_points_save<true>(p, stream) : launch_points_save<false>(p, stream);
    return vis ? launch_points_cfg<true>(p, vpw, a->arith, stream) : launch_points_cfg<false>(p, vpw, a->arith, stream);
}

int neuray_render_rays(const NeurayRaysArgs* a, void* stream) {
    if (!a) return fail("neuray_render_rays: null args");
    if (a->dn < 1 || a->dn > 4 * NEURAY_MAX_SAMPLES) return fail("neuray_render_rays: dn=%d unsupported", a->dn);
    nr::RayParams p;
    p.point_rec = a->point_rec_dev; p.depth = a->depth_dev; p.pos_enc = a->pos_enc_dev; p.weights = a->packed_weights_dev;
    p.hit_prob = a->hit_prob_dev; p.pixel = a->pixel_dev; p.render_depth = a->render_depth_dev; p.ray_mask = a->ray_mask_dev;
    p.density = a->density_dev; p.att_save = a->att_save_dev; p.rn = a->rn; p.dn = a->dn;
    p.mask_view_num = a->ray_mask_view_num; p.mask_point_num = a->ray_mask_point_num;
    // two rays per wave when a ray's samples fill at most half of one (the 32-sample fine pass of the headline configuration)
    const int rpw = a->dn <= 32 ? 2 : 1;
    const size_t smem = nr::ray_smem_bytes(a->dn, rpw);
    if (smem > 160 * 1024) return fail("neuray_render_rays: dn=%d needs %zu bytes of LDS", a->dn, smem);
    const int grid = grid_for(a->rn, nr::kRayWaves * rpw, 256 * 16);
    // (saved: the training forward - the attention's softmax statistics are kept for the backward)
    const auto k = a->att_save_dev ? (rpw == 2 ? nr::rays_kernel<true, 2> : nr::rays_kernel<true, 1>)
                                   : (rpw == 2 ? nr::rays_kernel<false, 2> : nr::rays_kernel<false, 1>);
    launch_lds(k, dim3(grid), dim3(64 * nr::kRayWaves), smem, stream, p);
    return check_launch("neuray_render_rays");
}

int neuray_sample_fine_depth(const float* query_const, const float* depth, const float* hit_prob, const float* u,
                             int rn, int dn, int fdn, int use_all, float* out, void* stream) {
    return neuray_sample_fine_depth_traced(query_const, depth, hit_prob, u, rn, dn, fdn, use_all, out, nullptr, nullptr, stream);
}

int neuray_sample_fine_depth_traced(const float* query_const, const float* depth, const float* hit_prob, const float* u,
                                    int rn, int dn, int fdn, int use_all, float* out, int* idx_out, float* cdf_out, void* stream) {
    if (dn < 2 || dn > NEURAY_MAX_SAMPLES || fdn < 1 || fdn > NEURAY_MAX_SAMPLES)
        return fail("neuray_sample_fine_depth: dn=%d fdn=%d outside [2,%d]", dn, fdn, NEURAY_MAX_SAMPLES);
    nr::FineParams p;
    p.que_const = query_const; p.depth = depth; p.hit_prob = hit_prob; p.u = u; p.out = out; p.idx_out = idx_out; p.cdf_out = cdf_out;
    p.rn = rn; p.dn = dn; p.fdn = fdn; p.use_all = use_all & 1; p.no_sort = (use_all >> 1) & 1; p.linear = (use_all >> 2) & 1;
    const int grid = grid_for(rn, nr::kRayWaves, 256 * 16);
    NR_LAUNCH(nr::fine_kernel, dim3(grid), dim3(64 * nr::kRayWaves), 0, stream, p);
    return check_launch("neuray_sample_fine_depth");
}

int neuray_interpolate_feats(const float* feats, const float* points, const float* mask, int b, int n, int c, int fh, int fw,
                             int h_full, int w_full, int align_corners, float* out, void* stream) {
    if (b < 1 || n < 1 || c < 1) return fail("neuray_interpolate_feats: bad shape b=%d n=%d c=%d", b, n, c);
    const int grid = grid_for((long long)b * n * c, 256, 256 * 8);
    NR_LAUNCH(nr::interpolate_kernel, dim3(grid), dim3(256), 0, stream, feats, points, mask, b, n, c, fh, fw, h_full, w_full,
              align_corners, out);
    return check_launch("neuray_interpolate_feats");
}

int neuray_diff_feats(const float* view_const, const float* lift_const, const float* rgbd, int rfn, int h, int w, float* out, void* stream) {
    if (!view_const || !lift_const || !rgbd || !out) return fail("neuray_diff_feats: null pointer");
    if (rfn < 1 || rfn > NEURAY_MAX_VIEWS || h < 2 || w < 2) return fail("neuray_diff_feats: bad shape rfn=%d h=%d w=%d", rfn, h, w);
    nr::DiffFeatsParams p;
    p.view_const = view_const; p.lift_const = lift_const; p.rgbd = rgbd; p.out = out; p.rfn = rfn; p.h = h; p.w = w;
    const int grid = grid_for((long long)rfn * h * w, 256, 256 * 32);
    NR_LAUNCH(nr::diff_feats_kernel, dim3(grid), dim3(256), 0, stream, p);
    return check_launch("neuray_diff_feats");
}

int neuray_warp_variance(const float* ref_feats, const float* src_feats, const int* nn_ids, const float* transforms, const float* depth_vals,
                         int rfn, int sn, int n_num, int dn, int fh, int fw, float* out, void* stream) {
    return neuray_warp_variance_layout(ref_feats, src_feats, nn_ids, transforms, depth_vals, rfn, sn, n_num, dn, fh, fw, 0, out, stream);
}

int neuray_conv3d_c32_c8(const float* x_ndhwc, const float* wpack, const float* bias, float slope, int n, int d, int h, int w, float* out, void* stream) {
    if (!x_ndhwc || !wpack || !bias || !out) return fail("neuray_conv3d_c32_c8: null pointer");
    if (n < 1 || d < 1 || h < 1 || w < 1 || (long long)d * h * w * 128 >= 0x7fffff00LL)
        return fail("neuray_conv3d_c32_c8: bad shape n=%d d=%d h=%d w=%d (one image's volume must stay below 2^31 bytes)", n, d, h, w);
    nr::Conv0Params p;
    p.x = x_ndhwc; p.wpack = wpack; p.bias = bias; p.out = out; p.n = n; p.d = d; p.h = h; p.w = w; p.slope = slope;
    const long long strips = (long long)n * d * ((h + 1) / 2) * ((w + 15) / 16);       // a wave takes two output rows of a 16-voxel strip
    const int grid = grid_for(strips, nr::kConv0Waves, 256 * 8);
    const size_t smem = sizeof(float) * nr::kConv0PackFloats;                            // 72 KB: two workgroups per CU
    launch_lds(nr::costreg_conv0_kernel, dim3(grid), dim3(64 * nr::kConv0Waves), smem, stream, p, true);
    return check_launch("neuray_conv3d_c32_c8");
}

long long neuray_conv3x3_x3_pack_bytes(int cin, int cout) {
    if (cin < 32 || cout < 32 || cin % 32 || cout % 32) return -1;
    return (long long)9 * cin * cout * 6;
}

int neuray_conv3x3_x3_pack(const float* w, int cout, int cin, void* wpack, void* wpack_t, void* stream) {
    if (!w || (!wpack && !wpack_t)) return fail("neuray_conv3x3_x3_pack: null pointer");
    if (cin < 32 || cout < 32 || cin % 32 || cout % 32)
        return fail("neuray_conv3x3_x3_pack: (C_in, C_out) = (%d, %d): both must be multiples of 32", cin, cout);
    nr::Conv2dPackParams p;
    p.w = w; p.wpack = (unsigned*)wpack; p.wpack_t = (unsigned*)wpack_t; p.cout = cout; p.cin = cin;
    const int total = 9 * (cin / 32) * (cout / 16) * 256;
    NR_LAUNCH(nr::conv2d_x3_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, p);
    return check_launch("neuray_conv3x3_x3_pack");
}

namespace {
// relu: the entry point with the ReLU epilogue - the default tile shapes only (the NT / MTW overrides do not apply)
int conv3x3_x3_impl(bool relu, const float* x, const void* wpack, const float* bias, int n, int cin, int cout, int h, int w, int pad, float* out, void* stream) {
    if (!x || !wpack || !out) return fail("neuray_conv3x3_x3: null pointer");
    if (neuray_conv3x3_x3_pack_bytes(cin, cout) < 0)
        return fail("neuray_conv3x3_x3: (C_in, C_out) = (%d, %d): both must be multiples of 32", cin, cout);
    if (n < 1 || pad < 0 || pad > 2 || h + 2 * pad < 3 || w + 2 * pad < 3) return fail("neuray_conv3x3_x3: bad shape n=%d h=%d w=%d pad=%d", n, h, w, pad);
    const int oh = h + 2 * pad - 2, ow = w + 2 * pad - 2;
    if ((long long)n * cin * h * w * 4 >= 0x7fffff00LL || (long long)n * cout * oh * ow * 4 >= 0x7fffff00LL)
        return fail("neuray_conv3x3_x3: the input and the output must each stay below 2^31 bytes");
    static bool env_read = false;
    if (!env_read) {
        env_read = true;
        if (const char* e = getenv("NEURAY_CONV2D_NT")) g_conv2d_nt = atoi(e);
        if (const char* e = getenv("NEURAY_CONV2D_MTW")) g_conv2d_mtw = atoi(e);
    }
    // bands of at most 62 output columns (52-wide rows on 50 / 100 / 200-pixel maps: 2 dropped positions per row, a halo of 106 positions)
    const int tw_max = 62;
    const int bands = (ow + tw_max - 1) / tw_max;
    nr::Conv2dX3Params p;
    p.x = x; p.wpack = (const unsigned*)wpack; p.bias = bias; p.out = out; p.n = n; p.cin = cin; p.cout = cout; p.h = h; p.w = w; p.pad = pad;
    p.tw = (ow + bands - 1) / bands;
    const int mt = cout / 16;
    const long long q = (long long)n * (h + 2 * pad) * (p.tw + 2);
    if (q + 1024 >= 0x7fffffffLL) return fail("neuray_conv3x3_x3: n * (h + 2 pad) * (band width + 2) must stay below 2^31");
    // 64 positions x 32 output channels per wave: two workgroups per CU (70 KB of LDS each), the fastest shape on every encoder layer
    // (profiles/r06_zz5_conv2d_probes.log).  The larger tiles are reached only through NEURAY_CONV2D_NT / _MTW, which no tool sets any more:
    // they stay because the remaining kernels' code changes without them (profiles/r10_a_device_code_hashes.txt)
    int nt = 4, mtw = 2;
    if (g_conv2d_nt == 4 || g_conv2d_nt == 8) nt = g_conv2d_nt;
    if ((g_conv2d_mtw == 2 || g_conv2d_mtw == 4) && mt % g_conv2d_mtw == 0) mtw = g_conv2d_mtw;
    if ((size_t)nr::conv2d_x3_smem_bytes(nt, p.tw + 2) > 160 * 1024 || nr::conv2d_x3_positions(nt, p.tw + 2) > 64 * nr::conv2d_x3_max_passes(nt))
        return fail("neuray_conv3x3_x3: band of %d columns does not fit the LDS", p.tw);
    // two channel groups per workgroup where there are at least eight tiles of output channels: -7 % forward / -10 % data gradient at 128
    // channels, +-3 % at 64 (profiles/r06_zzf_conv2d_wc2.log)
    const bool wc2 = mt >= 8 && (mt / 2) % 2 == 0 && nr::conv2d_x3_positions(4, p.tw + 2) % 128 == 0;
    if (relu) {
        if ((size_t)nr::conv2d_x3_smem_bytes(4, p.tw + 2) > 160 * 1024 || nr::conv2d_x3_positions(4, p.tw + 2) > 64 * nr::conv2d_x3_max_passes(4))
            return fail("neuray_conv3x3_x3: band of %d columns does not fit the LDS", p.tw);
        if (wc2) launch_conv2d_x3<4, 2, 2, true>(p, bands, stream);
        else launch_conv2d_x3<4, 2, 1, true>(p, bands, stream);
        return check_launch("neuray_conv3x3_x3_relu");
    }
    if (nt == 8 && mtw == 4) launch_conv2d_x3<8, 4>(p, bands, stream);
    else if (nt == 8) launch_conv2d_x3<8, 2>(p, bands, stream);
    else if (mtw == 4) launch_conv2d_x3<4, 4>(p, bands, stream);
    else if (wc2) launch_conv2d_x3<4, 2, 2>(p, bands, stream);
    else launch_conv2d_x3<4, 2>(p, bands, stream);
    return check_launch("neuray_conv3x3_x3");
}
}  // namespace

int neuray_conv3x3_x3(const float* x, const void* wpack, const float* bias, int n, int cin, int cout, int h, int w, int pad, float* out, void* stream) {
    return conv3x3_x3_impl(false, x, wpack, bias, n, cin, cout, h, w, pad, out, stream);
}

int neuray_conv3x3_x3_relu(const float* x, const void* wpack, const float* bias, int n, int cin, int cout, int h, int w, int pad, float* out, void* stream) {
    return conv3x3_x3_impl(true, x, wpack, bias, n, cin, cout, h, w, pad, out, stream);
}

namespace {
int conv2d_wrw_ksplit(int n, int cin, int cout, int hp, int wp) {
    const int pairs = (cin / 32) * (cout / 32);
    const long long nkb = (long long)n * (((long long)(hp - 2) * wp + 31) / 32);
    long long ks = 512 / pairs;                     // two workgroups per CU over the whole launch ...
    if (ks > nkb / 8) ks = nkb / 8;                 // ... but at least two K blocks per wave
    return ks < 1 ? 1 : (int)ks;
}
}  // namespace

long long neuray_conv3x3_x3_wrw_workspace_floats(int n, int cin, int cout, int hp, int wp) {
    if (cin < 32 || cout < 32 || cin % 32 || cout % 32 || n < 1 || hp < 3 || wp < 10 || (wp & 1)) return -1;
    return (long long)conv2d_wrw_ksplit(n, cin, cout, hp, wp) * (cin / 32) * (cout / 32) * nr::kWrwAcc * 64;
}

int neuray_conv3x3_x3_wrw(const float* dy, const float* xp, int n, int cin, int cout, int hp, int wp, float* workspace, float* dw, void* stream) {
    if (!dy || !xp || !workspace || !dw) return fail("neuray_conv3x3_x3_wrw: null pointer");
    if (neuray_conv3x3_x3_wrw_workspace_floats(n, cin, cout, hp, wp) < 0)
        return fail("neuray_conv3x3_x3_wrw: n=%d (C_in, C_out) = (%d, %d) padded input %d x %d: the channel counts must be multiples of 32 and the padded width even and >= 10",
                    n, cin, cout, hp, wp);
    if ((long long)n * cin * hp * wp * 4 >= 0x7fffff00LL || (long long)n * cout * hp * wp * 4 >= 0x7fffff00LL)
        return fail("neuray_conv3x3_x3_wrw: the input and the output gradient must each stay below 2^31 bytes");
    nr::Conv2dWrwParams p;
    p.dy = dy; p.xp = xp; p.ws = workspace; p.dw = dw; p.n = n; p.cin = cin; p.cout = cout; p.hp = hp; p.wp = wp;
    p.ksplit = conv2d_wrw_ksplit(n, cin, cout, hp, wp);
    const int pairs = (cin / 32) * (cout / 32);
    const size_t smem = sizeof(float) * 2 * nr::kWrwAcc * 64;
    launch_lds(nr::conv2d_x3_wrw_kernel, dim3((unsigned)p.ksplit, (unsigned)pairs), dim3(256), smem, stream, p, true);
    NR_LAUNCH(nr::conv2d_x3_wrw_reduce_kernel, dim3((unsigned)(pairs * nr::kWrwAcc)), dim3(64 * nr::kWrwRedWaves), 0, stream, p);
    return check_launch("neuray_conv3x3_x3_wrw");
}

int neuray_convtranspose3d_bn_leaky(const float* x, const float* wpack, const float* bias, float slope, const float* skip, int n, int cin, int cout,
                                    int d, int h, int w, float* out, void* stream) {
    if (!x || !wpack || !bias || !out) return fail("neuray_convtranspose3d_bn_leaky: null pointer");
    const long long groups = (long long)(((long long)h * w + 255) / 256) * d * n;      // one thread per input voxel = 2 x 2 x 2 output block
    if (n < 1 || d < 1 || h < 1 || w < 1 || groups > 0x7fffffffLL)
        return fail("neuray_convtranspose3d_bn_leaky: bad shape n=%d d=%d h=%d w=%d", n, d, h, w);
    nr::Up11Params p;
    p.x = x; p.wpack = wpack; p.bias = bias; p.skip = skip; p.out = out; p.n = n; p.d = d; p.h = h; p.w = w; p.slope = slope;
    if (cin == 16 && cout == 8) NR_LAUNCH((nr::costreg_up11_kernel<16, 8>), dim3((unsigned)groups, 8 / nr::kUp11Co), dim3(256), 0, stream, p);
    else if (cin == 32 && cout == 16) NR_LAUNCH((nr::costreg_up11_kernel<32, 16>), dim3((unsigned)groups, 16 / nr::kUp11Co), dim3(256), 0, stream, p);
    else return fail("neuray_convtranspose3d_bn_leaky: (C_in, C_out) = (%d, %d) is not built (16 -> 8, 32 -> 16)", cin, cout);
    return check_launch("neuray_convtranspose3d_bn_leaky");
}

int neuray_convtranspose3d_c16_c8(const float* x, const float* wpack, const float* bias, float slope, const float* skip, int n, int d, int h, int w,
                                  float* out, void* stream) {
    return neuray_convtranspose3d_bn_leaky(x, wpack, bias, slope, skip, n, 16, 8, d, h, w, out, stream);
}

int neuray_conv3d_c8_c1(const float* x, const float* w27, float bias, int n, int d, int h, int w, float* out, void* stream) {
    if (!x || !w27 || !out) return fail("neuray_conv3d_c8_c1: null pointer");
    if (n < 1 || d < 1 || h < 1 || w < 1) return fail("neuray_conv3d_c8_c1: bad shape n=%d d=%d h=%d w=%d", n, d, h, w);
    nr::ProbParams p;
    p.x = x; p.w = w27; p.out = out; p.n = n; p.d = d; p.h = h; p.w_ = w; p.bias = bias;
    const long long grid = (long long)((h * w + 255) / 256) * ((d + nr::kProbSeg - 1) / nr::kProbSeg) * n;
    if (grid > 0x7fffffffLL) return fail("neuray_conv3d_c8_c1: volume too large");
    NR_LAUNCH(nr::costreg_prob_kernel, dim3((unsigned)grid), dim3(256), 0, stream, p);
    return check_launch("neuray_conv3d_c8_c1");
}

int neuray_conv3d_bn_leaky(const float* x, const float* wpack, const float* bias, float slope, int n, int cin, int cout, int stride, int d,
                           int h, int w, float* out, void* stream) {
    if (!x || !wpack || !bias || !out) return fail("neuray_conv3d_bn_leaky: null pointer");
    if (n < 1 || d < 1 || h < 1 || w < 1) return fail("neuray_conv3d_bn_leaky: bad shape n=%d d=%d h=%d w=%d", n, d, h, w);
    if ((long long)cin * d * h * w * 4 >= 0x7fffff00LL) return fail("neuray_conv3d_bn_leaky: one image's input volume must stay below 2^31 bytes");
    if (stride != 1 && stride != 2) return fail("neuray_conv3d_bn_leaky: stride %d", stride);
    nr::Conv3dParams p;
    p.x = x; p.wpack = wpack; p.bias = bias; p.out = out; p.n = n; p.d = d; p.h = h; p.w = w; p.slope = slope; p.cin = cin; p.cout = cout;
    const int od = (d - 1) / stride + 1, oh = (h - 1) / stride + 1, ow = (w - 1) / stride + 1;
    const long long tasks = (long long)n * od * ((oh + nr::kC3Rows - 1) / nr::kC3Rows) * ((ow + 15) / 16);
    const dim3 grid(grid_for(tasks, nr::kC3Waves, 256 * 16)), block(64 * nr::kC3Waves);
    // the kernel's channel counts: C_in rounded up to a multiple of 4, C_out to a multiple of 16 (wpack / bias are padded with zeros to them)
    const int ci = (cin + 3) / 4 * 4, co = (cout + 15) / 16 * 16;
    if (ci == 16 && co == 16 && stride == 1) NR_LAUNCH((nr::conv3d_kernel<16, 16, 1>), grid, block, 0, stream, p);
    else if (ci == 32 && co == 32 && stride == 1) NR_LAUNCH((nr::conv3d_kernel<32, 32, 1>), grid, block, 0, stream, p);
    else if (ci == 8 && co == 16 && stride == 2) NR_LAUNCH((nr::conv3d_kernel<8, 16, 2>), grid, block, 0, stream, p);
    else if (ci == 16 && co == 32 && stride == 2) NR_LAUNCH((nr::conv3d_kernel<16, 32, 2>), grid, block, 0, stream, p);
    else if (ci == 4 && co == 16 && stride == 1) NR_LAUNCH((nr::conv3d_kernel<4, 16, 1>), grid, block, 0, stream, p);
    else if (ci == 8 && co == 16 && stride == 1) NR_LAUNCH((nr::conv3d_kernel<8, 16, 1>), grid, block, 0, stream, p);
    else return fail("neuray_conv3d_bn_leaky: (C_in, C_out, stride) = (%d, %d, %d) is not built (padded to multiples of 4 / 16: 4 | 8 | 16 -> 16 and 32 -> 32 at "
                     "stride 1, 8 -> 16 and 16 -> 32 at stride 2)", cin, cout, stride);
    return check_launch("neuray_conv3d_bn_leaky");
}

int neuray_scale_shift_leaky(float* x, const float* scale, const float* shift, int n, int c, long long inner, float slope, void* stream) {
    if (!x || !scale || !shift) return fail("neuray_scale_shift_leaky: null pointer");
    if (n < 1 || c < 1 || inner < 1 || (long long)n * c > 0x7fffffffLL) return fail("neuray_scale_shift_leaky: bad shape n=%d c=%d inner=%lld", n, c, inner);
    nr::ScaleShiftLeakyParams p;
    p.x = x; p.scale = scale; p.shift = shift; p.inner = inner; p.n = n; p.c = c; p.slope = slope;
    const long long planes = (long long)n * c;
    if (planes > 65535) return fail("neuray_scale_shift_leaky: %lld planes exceed the grid's y range", planes);
    long long chunks = (4096 + planes - 1) / planes, most = (inner / 4 + 255) / 256;     // ~4096 workgroups, each thread >= one 16-byte piece
    if (chunks > most) chunks = most;
    if (chunks < 1) chunks = 1;
    NR_LAUNCH(nr::scale_shift_leaky_kernel, dim3((unsigned)chunks, (unsigned)planes), dim3(256), 0, stream, p);
    return check_launch("neuray_scale_shift_leaky");
}

int neuray_warp_variance_layout(const float* ref_feats, const float* src_feats, const int* nn_ids, const float* transforms, const float* depth_vals,
                                int rfn, int sn, int n_num, int dn, int fh, int fw, int channels_last, float* out, void* stream) {
    if (!ref_feats || !src_feats || !nn_ids || !transforms || !depth_vals || !out) return fail("neuray_warp_variance: null pointer");
    if (rfn < 1 || sn < 1 || n_num < 1 || dn < 1 || fh < 2 || fw < 2)
        return fail("neuray_warp_variance: bad shape rfn=%d sn=%d n_num=%d dn=%d fh=%d fw=%d", rfn, sn, n_num, dn, fh, fw);
    nr::WarpVarParams p;
    p.ref_feats = ref_feats; p.src_feats = src_feats; p.nn_ids = nn_ids; p.transforms = transforms; p.depth_vals = depth_vals; p.out = out;
    p.rfn = rfn; p.n_num = n_num; p.dn = dn; p.fh = fh; p.fw = fw; p.channels_last = channels_last;
    if (channels_last && (long long)rfn * dn <= 65535) {        // eight lanes per voxel, a tap = one 128-byte line per instruction
        NR_LAUNCH(nr::warp_variance_cl_kernel, dim3((fh * fw + 31) / 32, rfn * dn), dim3(256), 0, stream, p);
        return check_launch("neuray_warp_variance (channels last)");
    }
    const int grid = grid_for((long long)rfn * dn * fh * fw, 256, 256 * 64);
    NR_LAUNCH(nr::warp_variance_kernel, dim3(grid), dim3(256), 0, stream, p);
    return check_launch("neuray_warp_variance");
}

// ---- fused InstanceNorm + activation (+ residual) + reflection pad of the per-image encoders (nr_kernels_norm.h) ----------------
// One launcher per direction.  `who` is the exported symbol the caller invoked; `partials` selects the form: NULL = the atomic statistics
// (raw zeroed by the caller), else the deterministic ones (every workgroup's pair to partials, inorm_finish_kernel adds
// them into raw in workgroup order).
namespace {
int norm_chunks(int planes, int hw) {          // workgroups per plane: ~4096 workgroups in all (16 per CU), each thread >= 4 elements
    int want = (4096 + planes - 1) / planes, most = (hw + 1023) / 1024;
    if (want > most) want = most;
    return want < 1 ? 1 : want;
}

// the shape and stride check of the four norm entries (a stride of 0 = dense images)
int norm_check(const char* who, int n, int c, int h, int w, int pad, int act, long long stride_a, long long stride_b) {
    if (n < 1 || c < 1 || h < 1 || w < 1 || pad < 0 || pad >= h || pad >= w || act < 0 || act > 2 || (long long)(h + 2 * pad) * (w + 2 * pad) >= (1 << 23))
        return fail("%s: bad arguments n=%d c=%d h=%d w=%d pad=%d act=%d", who, n, c, h, w, pad, act);
    const long long img = (long long)c * (h + 2 * pad) * (w + 2 * pad);
    if ((stride_a != 0 && stride_a < img) || (stride_b != 0 && stride_b < img))
        return fail("%s: image strides %lld / %lld < %lld", who, stride_a, stride_b, img);
    return 0;
}

void norm_finish(const float* partials, int planes, int chunks, float* raw, void* stream) {
    NR_LAUNCH(nr::inorm_finish_kernel, dim3((2 * planes + 255) / 256), dim3(256), 0, stream, partials, planes, chunks, raw);
}

int inorm_forward(const char* who, const float* x, const float* gamma, const float* beta, const float* res, long long res_stride_n,
                  long long res_stride_c, long long res_stride_h, int n, int c, int h, int w, int pad, int act, float eps, float* partials,
                  float* raw, float* stats, float* out_padded, long long out_stride_n, void* stream) {
    if (!x || !gamma || !beta || !raw || !stats || !out_padded) return fail("%s: null pointer", who);
    if (int rc = norm_check(who, n, c, h, w, pad, act, out_stride_n, 0)) return rc;
    const long long img = (long long)c * (h + 2 * pad) * (w + 2 * pad);
    const int planes = n * c, hw = h * w, chunks = norm_chunks(planes, hw);
    if (partials) {
        NR_LAUNCH(nr::inorm_stats_kernel<true>, dim3(chunks, planes), dim3(256), 0, stream, x, hw, partials);
        norm_finish(partials, planes, chunks, raw, stream);
    } else {
        NR_LAUNCH(nr::inorm_stats_kernel<false>, dim3(chunks, planes), dim3(256), 0, stream, x, hw, raw);
    }
    nr::NormApplyParams p;
    p.x = x; p.raw = raw; p.gamma = gamma; p.beta = beta; p.res = res; p.out = out_padded; p.stats = stats;
    p.rs_n = res_stride_n; p.rs_c = res_stride_c; p.rs_h = res_stride_h; p.out_stride_n = out_stride_n ? out_stride_n : img;
    p.n = n; p.c = c; p.h = h; p.w = w; p.pad = pad; p.act = act; p.eps = eps;
    NR_LAUNCH(nr::inorm_apply_kernel, dim3(norm_chunks(planes, (h + 2 * pad) * (w + 2 * pad)), planes), dim3(256), 0, stream, p);
    return check_launch(who);
}

int inorm_backward(const char* who, const float* x, const float* out_padded, long long out_stride_n, const float* d_out_padded,
                   long long d_out_stride_n, const float* stats, const float* gamma, int n, int c, int h, int w, int pad, int act,
                   float* partials, float* raw, float* dx, float* d_res, float* d_gamma, float* d_beta, void* stream) {
    if (!x || !out_padded || !d_out_padded || !stats || !gamma || !raw || !dx) return fail("%s: null pointer", who);
    if (int rc = norm_check(who, n, c, h, w, pad, act, out_stride_n, d_out_stride_n)) return rc;
    const long long img = (long long)c * (h + 2 * pad) * (w + 2 * pad);
    nr::NormBwdParams p;
    p.x = x; p.out = out_padded; p.d_out = d_out_padded; p.stats = stats; p.gamma = gamma; p.dx = dx; p.d_res = d_res;
    p.d_gamma = d_gamma; p.d_beta = d_beta; p.raw = partials ? partials : raw;
    p.out_stride_n = out_stride_n ? out_stride_n : img; p.d_out_stride_n = d_out_stride_n ? d_out_stride_n : img;
    p.n = n; p.c = c; p.h = h; p.w = w; p.pad = pad; p.act = act;
    const int planes = n * c, hw = h * w, chunks = norm_chunks(planes, hw);
    if (partials) {
        NR_LAUNCH(nr::inorm_backward_reduce_kernel<true>, dim3(chunks, planes), dim3(256), 0, stream, p);
        norm_finish(partials, planes, chunks, raw, stream);
        p.raw = raw;
    } else {
        NR_LAUNCH(nr::inorm_backward_reduce_kernel<false>, dim3(chunks, planes), dim3(256), 0, stream, p);
    }
    NR_LAUNCH(nr::inorm_backward_apply_kernel, dim3(chunks, planes), dim3(256), 0, stream, p);
    return check_launch(who);
}
}  // namespace

int neuray_inorm_forward(const float* x, const float* gamma, const float* beta, const float* res, long long res_stride_n,
                         long long res_stride_c, long long res_stride_h, int n, int c, int h, int w, int pad, int act, float eps,
                         float* raw_zeroed, float* stats, float* out_padded, long long out_stride_n, void* stream) {
    return inorm_forward("neuray_inorm_forward", x, gamma, beta, res, res_stride_n, res_stride_c, res_stride_h, n, c, h, w, pad, act, eps,
                         nullptr, raw_zeroed, stats, out_padded, out_stride_n, stream);
}

int neuray_inorm_forward_det(const float* x, const float* gamma, const float* beta, const float* res, long long res_stride_n,
                             long long res_stride_c, long long res_stride_h, int n, int c, int h, int w, int pad, int act, float eps,
                             float* partials, float* raw, float* stats, float* out_padded, long long out_stride_n, void* stream) {
    if (!partials) return fail("neuray_inorm_forward_det: null pointer");
    return inorm_forward("neuray_inorm_forward_det", x, gamma, beta, res, res_stride_n, res_stride_c, res_stride_h, n, c, h, w, pad, act, eps,
                         partials, raw, stats, out_padded, out_stride_n, stream);
}

int neuray_inorm_backward(const float* x, const float* out_padded, long long out_stride_n, const float* d_out_padded, long long d_out_stride_n,
                          const float* stats, const float* gamma, int n, int c, int h, int w, int pad, int act, float* raw_zeroed, float* dx,
                          float* d_res, float* d_gamma, float* d_beta, void* stream) {
    return inorm_backward("neuray_inorm_backward", x, out_padded, out_stride_n, d_out_padded, d_out_stride_n, stats, gamma, n, c, h, w, pad, act,
                          nullptr, raw_zeroed, dx, d_res, d_gamma, d_beta, stream);
}

int neuray_inorm_backward_det(const float* x, const float* out_padded, long long out_stride_n, const float* d_out_padded, long long d_out_stride_n,
                              const float* stats, const float* gamma, int n, int c, int h, int w, int pad, int act, float* partials, float* raw,
                              float* dx, float* d_res, float* d_gamma, float* d_beta, void* stream) {
    if (!partials) return fail("neuray_inorm_backward_det: null pointer");
    return inorm_backward("neuray_inorm_backward_det", x, out_padded, out_stride_n, d_out_padded, d_out_stride_n, stats, gamma, n, c, h, w, pad,
                          act, partials, raw, dx, d_res, d_gamma, d_beta, stream);
}

int neuray_upsample2x_pad_forward(const float* x, int planes, int h, int w, int pad, float scale_y, float scale_x, float* out_padded, void* stream) {
    if (!x || !out_padded) return fail("neuray_upsample2x_pad_forward: null pointer");
    if (planes < 1 || h < 2 || w < 2 || pad < 0 || pad > 1 || (long long)(2 * h + 2 * pad) * (2 * w + 2 * pad) >= (1 << 23))
        return fail("neuray_upsample2x_pad_forward: bad arguments planes=%d h=%d w=%d pad=%d", planes, h, w, pad);
    nr::UpsampleParams p;
    p.x = x; p.out = out_padded; p.planes = planes; p.h = h; p.w = w; p.pad = pad; p.sy = scale_y; p.sx = scale_x;
    NR_LAUNCH(nr::upsample2x_pad_kernel, dim3(norm_chunks(planes, (2 * h + 2 * pad) * (2 * w + 2 * pad)), planes), dim3(256), 0, stream, p);
    return check_launch("neuray_upsample2x_pad_forward");
}

int neuray_upsample2x_pad_backward(const float* d_out_padded, int planes, int h, int w, int pad, const int* cnt_y, const int* idx_y,
                                   const float* wgt_y, const int* cnt_x, const int* idx_x, const float* wgt_x, float* dx, void* stream) {
    if (!d_out_padded || !cnt_y || !idx_y || !wgt_y || !cnt_x || !idx_x || !wgt_x || !dx) return fail("neuray_upsample2x_pad_backward: null pointer");
    if (planes < 1 || h < 2 || w < 2 || w > 2047 || pad < 0 || pad > 1 || (long long)h * w >= (1 << 23))
        return fail("neuray_upsample2x_pad_backward: bad arguments planes=%d h=%d w=%d (<= 2047) pad=%d", planes, h, w, pad);
    nr::UpsampleBwdParams p;
    p.d_out = d_out_padded; p.dx = dx; p.cnt_y = cnt_y; p.idx_y = idx_y; p.wgt_y = wgt_y; p.cnt_x = cnt_x; p.idx_x = idx_x; p.wgt_x = wgt_x;
    p.planes = planes; p.h = h; p.w = w; p.hp = 2 * h + 2 * pad; p.wp = 2 * w + 2 * pad;
    NR_LAUNCH(nr::upsample2x_pad_backward_kernel, dim3((h + nr::kUpRows - 1) / nr::kUpRows, planes), dim3(256),
              sizeof(float) * nr::kUpRows * (size_t)p.wp, stream, p);
    return check_launch("neuray_upsample2x_pad_backward");
}

int neuray_rays_points(const float* query_const, const float* coords, const float* depth, int rn, int dn, float* centers,
                       float* dirs, float* pts, float* que_dir, void* stream) {
    if (rn < 1 || (pts && (dn < 1 || !depth || !que_dir))) return fail("neuray_rays_points: bad arguments rn=%d dn=%d", rn, dn);
    const int grid = grid_for((long long)rn * (pts ? dn : 1), 256, 256 * 8);
    NR_LAUNCH(nr::rays_points_kernel, dim3(grid), dim3(256), 0, stream, query_const, coords, depth, rn, dn, centers, dirs, pts, que_dir);
    return check_launch("neuray_rays_points");
}

int neuray_depth_dists(const float* depth, const float* que_depth_range, int inverse, int rows, int dn, float* out, void* stream) {
    if (rows < 1 || dn < 1 || (inverse && !que_depth_range)) return fail("neuray_depth_dists: bad arguments");
    const int grid = grid_for((long long)rows * dn, 256, 256 * 8);
    NR_LAUNCH(nr::dists_kernel, dim3(grid), dim3(256), 0, stream, depth, que_depth_range, inverse, rows, dn, out);
    return check_launch("neuray_depth_dists");
}

int neuray_project_points(const float* view_const, const float* pts, int rfn, int pn, int h, int w, float* dir, float* pts2d,
                          float* depth, unsigned char* mask, void* stream) {
    if (rfn < 1 || pn < 1) return fail("neuray_project_points: bad shape rfn=%d pn=%d", rfn, pn);
    const int grid = grid_for((long long)rfn * pn, 256, 256 * 8);
    NR_LAUNCH(nr::project_kernel, dim3(grid), dim3(256), 0, stream, view_const, pts, rfn, pn, h, w, dir, pts2d, depth, mask);
    return check_launch("neuray_project_points");
}

int neuray_alpha2hit_prob(const float* alpha, int rows, int dn, float* out, void* stream) {
    if (rows < 1 || dn < 1) return fail("neuray_alpha2hit_prob: bad shape");
    const int grid = grid_for(rows, 64, 256 * 8);
    NR_LAUNCH(nr::hit_prob_kernel, dim3(grid), dim3(64), 0, stream, alpha, rows, dn, out);
    return check_launch("neuray_alpha2hit_prob");
}

int neuray_direct_render_points(const float* query_const, const float* view_const, const float* coords, const float* depth,
                                const float* rgba, const float* view_rec, const float* regs, int rfn, int rn, int dn, int h, int w,
                                float ground, float* alpha, float* color, void* stream) {
    if (rfn < 1 || rfn > NEURAY_MAX_VIEWS || rn < 1 || dn < 1) return fail("neuray_direct_render_points: bad shape rfn=%d rn=%d dn=%d", rfn, rn, dn);
    if (!view_rec || !alpha) return fail("neuray_direct_render_points: view_rec / alpha missing");
    const int grid = grid_for((long long)rn * dn, 128, 256 * 16);
    NR_LAUNCH(nr::dr_points_kernel, dim3(grid), dim3(128), 0, stream, query_const, view_const, coords, depth, rgba, view_rec, regs, rfn, rn,
              dn, h, w, ground, alpha, color);
    return check_launch("neuray_direct_render_points");
}

int neuray_direct_render_rays(const float* alpha, const float* colors, int color_stride, int color_first, int rn, int dn,
                              float* hit_prob, float* pixel, void* stream) {
    if (rn < 1 || dn < 1 || color_stride < 3 || color_first < 0) return fail("neuray_direct_render_rays: bad shape");
    const int grid = grid_for(rn, 64, 256 * 8);
    NR_LAUNCH(nr::dr_rays_kernel, dim3(grid), dim3(64), 0, stream, alpha, colors, color_stride, color_first, rn, dn, hit_prob, pixel);
    return check_launch("neuray_direct_render_rays");
}

int neuray_direct_render_rays_backward(const float* alpha, const float* colors, const float* d_pixel, const float* d_hit_prob, int rn, int dn,
                                       float* d_alpha, float* d_colors, void* stream) {
#ifdef NR_INFERENCE_ONLY
    (void)alpha; (void)colors; (void)d_pixel; (void)d_hit_prob; (void)rn; (void)dn; (void)d_alpha; (void)d_colors; (void)stream;
    return fail("neuray_direct_render_rays_backward: the bf16-operand library is inference only");
#else
    if (rn < 1 || dn < 1) return fail("neuray_direct_render_rays_backward: bad shape rn=%d dn=%d", rn, dn);
    if (!alpha || !colors || !d_pixel || !d_alpha || !d_colors) return fail("neuray_direct_render_rays_backward: missing array");
    const int grid = grid_for(rn, 64, 256 * 8);
    NR_LAUNCH(nr::dr_rays_backward_kernel, dim3(grid), dim3(64), 0, stream, alpha, colors, d_pixel, d_hit_prob, rn, dn, d_alpha, d_colors);
    return check_launch("neuray_direct_render_rays_backward");
#endif
}

int neuray_direct_render_points_backward(const float* query_const, const float* view_const, const float* coords, const float* depth,
                                         const float* rgba, const float* view_rec, const float* regs, const float* d_alpha,
                                         const float* d_colors, int rfn, int rn, int dn, int h, int w, int use_vis, float* d_dec,
                                         void* stream) {
#ifdef NR_INFERENCE_ONLY
    (void)query_const; (void)view_const; (void)coords; (void)depth; (void)rgba; (void)view_rec; (void)regs; (void)d_alpha; (void)d_colors;
    (void)rfn; (void)rn; (void)dn; (void)h; (void)w; (void)use_vis; (void)d_dec; (void)stream;
    return fail("neuray_direct_render_points_backward: the bf16-operand library is inference only");
#else
    if (rfn < 1 || rfn > NEURAY_MAX_VIEWS || rn < 1 || dn < 1 || h < 1 || w < 1)
        return fail("neuray_direct_render_points_backward: bad shape rfn=%d rn=%d dn=%d h=%d w=%d", rfn, rn, dn, h, w);
    if (!query_const || !view_const || !coords || !depth || !rgba || !view_rec || !regs || !d_dec)
        return fail("neuray_direct_render_points_backward: missing array");
    const int grid = grid_for((long long)rn * dn, 128, 256 * 16);
    NR_LAUNCH(nr::dr_points_backward_kernel, dim3(grid), dim3(128), 0, stream, query_const, view_const, coords, depth, rgba, view_rec, regs,
              d_alpha, d_colors, rfn, rn, dn, h, w, use_vis, d_dec);
    return check_launch("neuray_direct_render_points_backward");
#endif
}

int neuray_dist_decoder_rows(const float* feats, const float* packed_weights, int n, int has_vis_head, float var_bias,
                             float* mean, float* var, float* aw, float* vis, void* stream) {
    if (n < 1) return fail("neuray_dist_decoder_rows: n=%d", n);
    if (has_vis_head && !vis) return fail("neuray_dist_decoder_rows: vis output missing");
    const int grid = grid_for(n, 32 * 4, 256 * 8);
    if (has_vis_head) NR_LAUNCH(nr::decoder_rows_kernel<true>, dim3(grid), dim3(256), 0, stream, feats, packed_weights, n, var_bias, mean, var, aw, vis);
    else NR_LAUNCH(nr::decoder_rows_kernel<false>, dim3(grid), dim3(256), 0, stream, feats, packed_weights, n, var_bias, mean, var, aw, vis);
    return check_launch("neuray_dist_decoder_rows");
}

int neuray_self_hit_prob(const float* query_const, const float* depth, const float* mean, const float* var, const float* aw,
                         const float* vis, int rn, int dn, float* out, void* stream) {
    if (rn < 1 || dn < 2) return fail("neuray_self_hit_prob: bad shape rn=%d dn=%d", rn, dn);
    const int grid = grid_for((long long)rn * dn, 256, 256 * 8);
    NR_LAUNCH(nr::self_hit_prob_kernel, dim3(grid), dim3(256), 0, stream, query_const, depth, mean, var, aw, vis, rn, dn, out);
    return check_launch("neuray_self_hit_prob");
}

int neuray_mfma_selftest(const float* A, const float* B, float* D, void* stream) {
    NR_LAUNCH(nr::mfma_selftest_kernel, dim3(1), dim3(64), 0, stream, A, B, D);
    return check_launch("neuray_mfma_selftest");
}

int neuray_x3_selftest(const float* A, const float* B, float* D, float* parts, void* stream) {
    if (!A || !B || !D) return fail("neuray_x3_selftest: null pointer");
    NR_LAUNCH(nr::x3_selftest_kernel, dim3(1), dim3(64), 0, stream, A, B, D, parts);
    return check_launch("neuray_x3_selftest");
}

int neuray_allreduce_selftest(const float* x, float* y, int nw, void* stream) {
    if (!x || !y) return fail("neuray_allreduce_selftest: null pointer");
    if (nw < 1 || nw > 8) return fail("neuray_allreduce_selftest: nw=%d outside [1,8]", nw);
    const size_t smem = nr::allreduce_selftest_smem_bytes(nw);
    if (smem > 64 * 1024) allow_lds(nr::allreduce_selftest_kernel, smem);
    NR_LAUNCH(nr::allreduce_selftest_kernel, dim3(1), dim3(64 * nw), smem, stream, x, y, nw);
    return check_launch("neuray_allreduce_selftest");
}

int neuray_points_resident_workgroups(int arith, int rfn) {
#ifdef NEURAY_EMU
    (void)arith; (void)rfn;
    return 0;
#else
    if (rfn < 7 || rfn > 8) return -1;                 // (the headline shape: four waves of two views)
    int n = 0;
    hipError_t e;
    if (arith == NEURAY_ARITH_X3) {
#ifdef NR_BF16_QUADS
        return -1;
#else
        if (!nr::point_one_barrier<1>(4, nr::AR_X3)) return -1;      // (the product form at four waves: launch_points_own)
        auto k = nr::points_kernel<1, 2, false, 1, 512, NR_POINT_MINW_X3, false, false, nr::AR_X3, true>;
        const size_t smem = nr::point_smem_bytes<1>(4, nr::AR_X3, true);
        if (smem > 64 * 1024) allow_lds(k, smem);
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 256, smem);
#endif
    } else {
        auto k = nr::points_kernel<1, 2, false, 1, 512, NR_POINT_MINW, false, false, nr::AR_F32>;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 256, nr::point_smem_bytes<1>(4, nr::AR_F32));
    }
    return e == hipSuccess ? n : -1;
#endif
}

static_assert(NEURAY_PACKED_RAY_FLOATS == nr::kPackedRayFloats && NEURAY_RW_WQ == nr::RW_WQ && NEURAY_RW_WK == nr::RW_WK &&
              NEURAY_RW_WV == nr::RW_WV && NEURAY_RW_FC == nr::RW_FC && NEURAY_RW_LNW == nr::RW_LNW && NEURAY_RW_LNB == nr::RW_LNB &&
              NEURAY_RW_OG0W == nr::RW_OG0W && NEURAY_RW_OG0B == nr::RW_OG0B && NEURAY_RW_OG2W == nr::RW_OG2W &&
              NEURAY_RW_OG2B == nr::RW_OG2B, "abi");

// ---- one launcher per backward kernel.  Every backward kernel has two exported forms: the atomic one, and the deterministic one of
// cfg['hip_deterministic'] (the kernel instantiated with DET = true stores every workgroup's sums with plain stores to
// its row of a partials buffer, and reduce_partials adds the rows in workgroup order - no float atomics).  The *_det entry is its
// namesake's launcher with scratch: `who` is the exported symbol the caller invoked, a NULL `partials` selects the atomic form.
// neuray_deterministic_partials_floats sizes the partials by the grid helpers below: the launchers call the same ones.
namespace {
int rays_bwd_grid(int rn, int dn) { return grid_for(rn, nr::ray_bwd_waves(dn), 256 * 4); }      // (ray_bwd_waves: rays per workgroup)
int points_bwd_grid(int rn, int dn) { return grid_for((long long)rn * dn, 16, 256); }           // persistent: one workgroup per CU
int rows_bwd_grid(int n) { return grid_for(n, 16, 512); }                                       // the self-hit and the decoder-rows backward: a wave per 16 rows

int reduce_partials(const char* who, const float* partials, int g, long long n, float* out, void* stream) {
    NR_LAUNCH(nr::reduce_partials_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, stream, partials, g, n, out);
    return check_launch(who);
}

int rays_backward(const char* who, const NeurayRaysBwdArgs* a, float* partials, void* stream) {
    if (!a || !a->point_rec_dev || !a->depth_dev || !a->pos_enc_dev || !a->packed_weights_dev || !a->d_pixel_dev ||
        !a->d_point_rec_dev || !a->d_ray_weights_dev)
        return fail("%s: null argument", who);
    if (a->rn < 1) return fail("%s: rn=%d", who, a->rn);
    if (a->dn < 3 || a->dn > NEURAY_MAX_SAMPLES) return fail("%s: dn=%d outside [3,%d]", who, a->dn, NEURAY_MAX_SAMPLES);
    const bool det = partials != nullptr;
    nr::RayBwdParams p;
    p.point_rec = a->point_rec_dev; p.depth = a->depth_dev; p.pos_enc = a->pos_enc_dev; p.weights = a->packed_weights_dev;
    p.d_pixel = a->d_pixel_dev; p.d_hit_prob = a->d_hit_prob_dev; p.d_depth = a->d_render_depth_dev;
    p.d_point_rec = a->d_point_rec_dev; p.d_weights = det ? partials : a->d_ray_weights_dev; p.att_saved = a->att_saved_dev;
    p.rn = a->rn; p.dn = a->dn;
    const size_t smem = nr::ray_bwd_smem_bytes(a->dn, det);
    const int waves = nr::ray_bwd_waves(a->dn), grid = rays_bwd_grid(a->rn, a->dn);
    // one sample per lane up to 64 samples, two beyond
    const auto k = a->dn <= 64 ? (det ? nr::rays_backward_kernel<1, true> : nr::rays_backward_kernel<1, false>)
                               : (det ? nr::rays_backward_kernel<2, true> : nr::rays_backward_kernel<2, false>);
    launch_lds(k, dim3(grid), dim3(64 * waves), smem, stream, p);
    if (int rc = check_launch(who)) return rc;
    return det ? reduce_partials(who, partials, grid, nr::kPackedRayFloats, a->d_ray_weights_dev, stream) : 0;
}
}  // namespace

int neuray_render_rays_backward(const NeurayRaysBwdArgs* a, void* stream) { return rays_backward("neuray_render_rays_backward", a, nullptr, stream); }

int neuray_render_rays_backward_det(const NeurayRaysBwdArgs* a, float* partials_dev, void* stream) {
    if (!partials_dev) return fail("neuray_render_rays_backward_det: null argument");
    return rays_backward("neuray_render_rays_backward_det", a, partials_dev, stream);
}

size_t neuray_flat_pass_floats(void) { return (size_t)nr::kFlatPassFloats; }
size_t neuray_packed_t_floats(void) { return (size_t)nr::kPackedTFloats; }
size_t neuray_points_saved_floats(int npts) { return npts < 1 ? 0 : (size_t)((npts + 15) / 16) * nr::kSavedTileFloats; }
int neuray_pack_pass_t_index_map(int has_vis_head, int* index) {
    if (!index) return fail("neuray_pack_pass_t_index_map: null argument");
#ifdef NR_INFERENCE_ONLY
    return fail("neuray_pack_pass_t_index_map: the bf16-operand library is inference only");
#else
    const int rc = nr::pack_pass_t_index_map(has_vis_head != 0, index);
    return rc ? fail("neuray_pack_pass_t_index_map: tensor %d missing", rc - 1) : 0;
#endif
}
size_t neuray_flat_tensor_offset(int t) { return (t < 0 || t > nr::T_COUNT) ? (size_t)0 : (size_t)nr::tensor_offset(t); }

// The point backward is nr_kernels_bwd2.h: 8 waves x 1 view at two waves per SIMD, run as its two halves - tail, then front - with a
// hand-over buffer in between (NeurayPointsBwdArgs.handover_dev).  Round 3's second decomposition (4 waves x 2 views per wave) was retired
// in round 4; round 6 removed the first-version kernel (rfn 9..16: a view count no shipped configuration trains with) and the one-launch
// form of the resident kernel (299 spilled VGPRs, 0.92 against 0.63 ms per pass).
size_t neuray_points_backward_handover_floats(int npoints) {
#ifdef NR_INFERENCE_ONLY
    (void)npoints;
    return 0;
#else
    return npoints < 1 ? 0 : nr::point_bwd2_handover_floats(npoints);
#endif
}

namespace {
// partials / rows / keys: the scratch of the deterministic form (all three, or none for the atomic one).  The deterministic instantiation
// leaves the maps' gradients to neuray_points_backward_scatter: it does not read d_ray_feats / d_img_feats, and takes rows and keys in
// those two fields of the parameter struct.
int points_backward(const char* who, const NeurayPointsBwdArgs* a, float* partials, float* rows, int* keys, void* stream) {
    const bool det = partials != nullptr;
    if (!a || !a->query_const_dev || !a->view_const_dev || !a->coords_dev || !a->depth_dev || !a->ray_feats_nhwc_dev ||
        !a->img_feats_nhwc_dev || !a->rgba_dev || !a->flat_weights_dev || !a->d_point_rec_dev || !a->d_flat_weights_dev ||
        (det ? !rows || !keys : !a->d_ray_feats_nhwc_dev || !a->d_img_feats_nhwc_dev))
        return fail("%s: null argument", who);
    if (a->rfn < 1 || a->rfn > NEURAY_MAX_VIEWS) return fail("%s: rfn=%d outside [1,%d]", who, a->rfn, NEURAY_MAX_VIEWS);
    if (a->rn < 1 || a->dn < 3 || a->dn > NEURAY_MAX_SAMPLES) return fail("%s: rn=%d dn=%d", who, a->rn, a->dn);
#ifdef NR_INFERENCE_ONLY
    (void)stream;
    return fail("%s: the bf16-operand library is inference only", who);
#else
    if (a->rfn > nr::kB2Waves)
        return fail("%s: rfn=%d - the backward covers at most %d reference views (the forward kernels take %d)", who, a->rfn, nr::kB2Waves,
                    NEURAY_MAX_VIEWS);
    if (det && (long long)(a->rfn + 1) * a->fh * a->fw > 0x7fffffffLL) return fail("%s: the maps' texels do not fit a 32-bit sort key", who);
    if (!a->packed_weights_dev || !a->packed_t_weights_dev)
        return fail("%s: packed_weights_dev and packed_t_weights_dev are needed (neuray_pack_pass_weights / neuray_pack_pass_t_index_map)", who);
    if (!a->saved_dev) return fail("%s: saved_dev is NULL (run neuray_render_points with saved_dev on the same inputs first)", who);
    if (!a->handover_dev) return fail("%s: handover_dev is NULL (neuray_points_backward_handover_floats(rn * dn) floats of scratch)", who);
    nr::PointBwd2Params q;
    q.que_const = a->query_const_dev; q.view_const = a->view_const_dev; q.coords = a->coords_dev; q.depth = a->depth_dev;
    q.ray_feats = a->ray_feats_nhwc_dev; q.img_feats = a->img_feats_nhwc_dev; q.rgba = a->rgba_dev;
    q.weights = a->packed_weights_dev; q.weights_t = a->packed_t_weights_dev;
    q.d_point_rec = a->d_point_rec_dev; q.saved = a->saved_dev;
    q.d_ray_feats = det ? rows : a->d_ray_feats_nhwc_dev;
    q.d_img_feats = det ? reinterpret_cast<float*>(keys) : a->d_img_feats_nhwc_dev;
    q.rfn = a->rfn; q.rn = a->rn; q.dn = a->dn; q.h = a->h; q.w = a->w; q.fh = a->fh; q.fw = a->fw;
    q.use_vis = a->use_vis; q.var_bias = a->var_bias;
    q.handover = a->handover_dev;
    const int grid = points_bwd_grid(a->rn, a->dn);
    const size_t smem = nr::point_bwd2_smem_bytes();
    // (a vis head that compute_prob does not consume - the fine decoder's when the coarse decoder has use_vis = False, quirk A.9.2 -
    // has an identically zero gradient on this path: the kernel without the head is the same computation)
    const bool vis = a->has_vis_head && a->use_vis;
    using K = void (*)(nr::PointBwd2Params);
    const K tail = det ? (vis ? K(nr::points_backward2_kernel<true, nr::B2_TAIL, true>) : K(nr::points_backward2_kernel<false, nr::B2_TAIL, true>))
                       : (vis ? K(nr::points_backward2_kernel<true, nr::B2_TAIL>) : K(nr::points_backward2_kernel<false, nr::B2_TAIL>));
    const K front = det ? (vis ? K(nr::points_backward2_kernel<true, nr::B2_FRONT, true>) : K(nr::points_backward2_kernel<false, nr::B2_FRONT, true>))
                        : (vis ? K(nr::points_backward2_kernel<true, nr::B2_FRONT>) : K(nr::points_backward2_kernel<false, nr::B2_FRONT>));
    // two launches: tail, then front (nr_kernels_bwd2.h B2Part), with a half of the partials each
    float* const p_tail = partials;
    float* const p_front = det ? partials + (size_t)grid * nr::kFlatPassFloats : nullptr;
    q.d_flat = det ? p_tail : a->d_flat_weights_dev;
    launch_lds(tail, dim3(grid), dim3(64 * nr::kB2Waves), smem, stream, q, true);
    q.d_flat = det ? p_front : a->d_flat_weights_dev;
    launch_lds(front, dim3(grid), dim3(64 * nr::kB2Waves), smem, stream, q, true);
    if (int rc = check_launch(who)) return rc;
    if (!det) return 0;
    // each half has its own reduce launch, in stream order: tail's rows first, then front's
    if (int rc = reduce_partials(who, p_tail, grid, nr::kFlatPassFloats, a->d_flat_weights_dev, stream)) return rc;
    return reduce_partials(who, p_front, grid, nr::kFlatPassFloats, a->d_flat_weights_dev, stream);
#endif
}

int self_hit_backward(const char* who, const float* qc, const float* depth, const float* feats, const float* packed, const float* packed_t,
                      int has_vis_head, int use_vis, float var_bias, const float* d_hit, int rn, int dn, float* d_feats, float* d_flat,
                      float* partials, void* stream) {
#ifdef NR_INFERENCE_ONLY
    return fail("%s: the bf16-operand variant is inference only", who);
#else
    if (!qc || !depth || !feats || !packed || !packed_t || !d_hit || !d_feats || !d_flat) return fail("%s: null argument", who);
    if (rn < 1 || dn < 3 || dn > NEURAY_MAX_SAMPLES) return fail("%s: rn=%d dn=%d", who, rn, dn);
    const bool det = partials != nullptr, vis = has_vis_head && use_vis;          // (an unused vis head: zero gradient)
    nr::SelfHitBwd2Params p;
    p.que_const = qc; p.depth = depth; p.feats = feats; p.weights = packed; p.weights_t = packed_t; p.d_hit = d_hit;
    p.d_feats = d_feats; p.d_flat = det ? partials : d_flat; p.rn = rn; p.dn = dn; p.use_vis = use_vis; p.var_bias = var_bias;
    const int grid = rows_bwd_grid(rn);
    const auto k = det ? (vis ? nr::self_hit_backward2_kernel<true, true> : nr::self_hit_backward2_kernel<false, true>)
                       : (vis ? nr::self_hit_backward2_kernel<true, false> : nr::self_hit_backward2_kernel<false, false>);
    NR_LAUNCH(k, dim3(grid), dim3(64), 0, stream, p);
    if (int rc = check_launch(who)) return rc;
    return det ? reduce_partials(who, partials, grid, nr::kFlatPassFloats, d_flat, stream) : 0;
#endif
}

int rows_backward(const char* who, const float* feats, const float* packed, const float* packed_t, int n, int has_vis_head, float var_bias,
                  const float* d_mean, const float* d_var, const float* d_aw, const float* d_vis, float* d_feats, float* d_flat,
                  float* partials, void* stream) {
#ifdef NR_INFERENCE_ONLY
    return fail("%s: the bf16-operand variant is inference only", who);
#else
    if (!feats || !packed || !packed_t || !d_feats || !d_flat) return fail("%s: null argument", who);
    if (n < 1) return fail("%s: n=%d", who, n);
    const bool det = partials != nullptr, vis = has_vis_head && d_vis;            // (no gradient into the vis head: not run)
    nr::RowsBwd2Params p;
    p.feats = feats; p.weights = packed; p.weights_t = packed_t; p.d_mean = d_mean; p.d_var = d_var; p.d_aw = d_aw; p.d_vis = d_vis;
    p.d_feats = d_feats; p.d_flat = det ? partials : d_flat; p.n = n; p.var_bias = var_bias;
    // (a persistent grid: every workgroup ends with one atomicAdd per weight of the heads it ran - 2048 of them cost more in the flush than in the rows)
    const int grid = rows_bwd_grid(n);
    const auto k = det ? (vis ? nr::decoder_rows_backward2_kernel<true, true> : nr::decoder_rows_backward2_kernel<false, true>)
                       : (vis ? nr::decoder_rows_backward2_kernel<true, false> : nr::decoder_rows_backward2_kernel<false, false>);
    NR_LAUNCH(k, dim3(grid), dim3(64), 0, stream, p);
    if (int rc = check_launch(who)) return rc;
    return det ? reduce_partials(who, partials, grid, nr::kFlatPassFloats, d_flat, stream) : 0;
#endif
}
}  // namespace

int neuray_render_points_backward(const NeurayPointsBwdArgs* a, void* stream) {
    return points_backward("neuray_render_points_backward", a, nullptr, nullptr, nullptr, stream);
}

int neuray_render_points_backward_det(const NeurayPointsBwdArgs* a, float* partials_zeroed_dev, float* rows_dev, int* keys_dev, void* stream) {
    if (!partials_zeroed_dev) return fail("neuray_render_points_backward_det: null argument");
    return points_backward("neuray_render_points_backward_det", a, partials_zeroed_dev, rows_dev, keys_dev, stream);
}

int neuray_self_hit_prob_backward(const float* qc, const float* depth, const float* feats, const float* packed, const float* packed_t,
                                  int has_vis_head, int use_vis, float var_bias, const float* d_hit, int rn, int dn,
                                  float* d_feats, float* d_flat, void* stream) {
    return self_hit_backward("neuray_self_hit_prob_backward", qc, depth, feats, packed, packed_t, has_vis_head, use_vis, var_bias, d_hit, rn, dn,
                             d_feats, d_flat, nullptr, stream);
}

int neuray_self_hit_prob_backward_det(const float* qc, const float* depth, const float* feats, const float* packed, const float* packed_t,
                                      int has_vis_head, int use_vis, float var_bias, const float* d_hit, int rn, int dn,
                                      float* d_feats, float* d_flat, float* partials_zeroed_dev, void* stream) {
    if (!partials_zeroed_dev) return fail("neuray_self_hit_prob_backward_det: null argument");
    return self_hit_backward("neuray_self_hit_prob_backward_det", qc, depth, feats, packed, packed_t, has_vis_head, use_vis, var_bias, d_hit, rn,
                             dn, d_feats, d_flat, partials_zeroed_dev, stream);
}

int neuray_dist_decoder_rows_backward(const float* feats, const float* packed, const float* packed_t, int n, int has_vis_head,
                                      float var_bias, const float* d_mean, const float* d_var, const float* d_aw, const float* d_vis,
                                      float* d_feats, float* d_flat, void* stream) {
    return rows_backward("neuray_dist_decoder_rows_backward", feats, packed, packed_t, n, has_vis_head, var_bias, d_mean, d_var, d_aw, d_vis,
                         d_feats, d_flat, nullptr, stream);
}

int neuray_dist_decoder_rows_backward_det(const float* feats, const float* packed, const float* packed_t, int n, int has_vis_head,
                                          float var_bias, const float* d_mean, const float* d_var, const float* d_aw, const float* d_vis,
                                          float* d_feats, float* d_flat, float* partials_zeroed_dev, void* stream) {
    if (!partials_zeroed_dev) return fail("neuray_dist_decoder_rows_backward_det: null argument");
    return rows_backward("neuray_dist_decoder_rows_backward_det", feats, packed, packed_t, n, has_vis_head, var_bias, d_mean, d_var, d_aw, d_vis,
                         d_feats, d_flat, partials_zeroed_dev, stream);
}

int neuray_interpolate_feats_backward(const float* d_out, const float* points, const float* mask, int b, int n, int c, int fh,
                                      int fw, int h_full, int w_full, int align_corners, float* d_feats, void* stream) {
    if (!d_out || !points || !d_feats) return fail("neuray_interpolate_feats_backward: null argument");
    if (b < 1 || n < 1 || c < 1 || fh < 1 || fw < 1) return fail("neuray_interpolate_feats_backward: bad shape");
    NR_LAUNCH(nr::interpolate_backward_kernel, dim3(grid_for((long long)b * n * c, 256, 4096)), dim3(256), 0, stream, d_out, points,
              mask, b, n, c, fh, fw, h_full, w_full, align_corners, d_feats);
    return check_launch("neuray_interpolate_feats_backward");
}

int neuray_interpolate_feats_backward_staged(const float* d_out, const float* points, const float* mask, int b, int n, int c, int fh,
                                             int fw, int h_full, int w_full, int align_corners, float* tmp_nhwc_zeroed, float* d_feats, void* stream) {
    if (!d_out || !points || !d_feats || !tmp_nhwc_zeroed) return fail("neuray_interpolate_feats_backward_staged: null argument");
    if (b < 1 || n < 1 || c < 1 || fh < 1 || fw < 1 || (long long)b * ((c + 31) / 32) > 65535) return fail("neuray_interpolate_feats_backward_staged: bad shape");
    NR_LAUNCH(nr::interpolate_backward_nhwc_kernel, dim3(grid_for((long long)b * n * c, 256, 4096)), dim3(256), 0, stream, d_out, points,
              mask, b, n, c, fh, fw, h_full, w_full, align_corners, tmp_nhwc_zeroed);
    if (int rc = check_launch("neuray_interpolate_feats_backward_staged")) return rc;
    NR_LAUNCH(nr::nhwc_add_to_nchw_kernel, dim3((fh * fw + 31) / 32, ((c + 31) / 32) * b), dim3(256), 0, stream, tmp_nhwc_zeroed, fh * fw, c, d_feats);
    return check_launch("neuray_interpolate_feats_backward_staged");
}

// ---- the rest of the deterministic training backward (the *_det entries stand next to their namesakes above): the sizes
// of the scratch, the ordered reduction on its own, and the maps' gradients as a segmented sum over sorted keys
namespace {
int scatter_sorted(const nr::ScatterSortedParams& p, void* stream) {
    NR_LAUNCH(nr::scatter_sorted_kernel, dim3(grid_for(p.ntex, 4, 256 * 16)), dim3(256), 0, stream, p);
    return check_launch("scatter_sorted");
}
}  // namespace

size_t neuray_deterministic_partials_floats(int kernel, int rn, int dn) {
    if (rn < 1) return 0;
    switch (kernel) {
        case NEURAY_DET_RAYS: return dn < 1 ? 0 : (size_t)rays_bwd_grid(rn, dn) * nr::kPackedRayFloats;
#ifndef NR_INFERENCE_ONLY
        case NEURAY_DET_POINTS: return dn < 1 ? 0 : (size_t)2 * points_bwd_grid(rn, dn) * nr::kFlatPassFloats;       // (tail's rows, then front's)
        case NEURAY_DET_SELF_HIT: case NEURAY_DET_ROWS: return (size_t)rows_bwd_grid(rn) * nr::kFlatPassFloats;
#endif
        default: return 0;
    }
}

int neuray_reduce_partials(const float* partials_dev, int g, long long n, float* out_dev, void* stream) {
    if (!partials_dev || !out_dev) return fail("neuray_reduce_partials: null argument");
    if (g < 1 || n < 1) return fail("neuray_reduce_partials: g=%d n=%lld", g, n);
    return reduce_partials("neuray_reduce_partials", partials_dev, g, n, out_dev, stream);
}

long long neuray_points_backward_scatter_columns(int npoints) {
#ifdef NR_INFERENCE_ONLY
    (void)npoints;
    return 0;
#else
    return npoints < 1 ? 0 : (long long)((npoints + 15) / 16) * 16 * nr::kB2Waves;
#endif
}

int neuray_points_backward_scatter(const int* sorted_keys_dev, const long long* perm_dev, const float* rows_dev, long long columns, int rfn,
                                   int fh, int fw, float* d_ray_feats_nhwc_dev, float* d_img_feats_nhwc_dev, void* stream) {
#ifdef NR_INFERENCE_ONLY
    return fail("neuray_points_backward_scatter: the bf16-operand library is inference only");
#else
    if (!sorted_keys_dev || !perm_dev || !rows_dev || !d_ray_feats_nhwc_dev || !d_img_feats_nhwc_dev) return fail("neuray_points_backward_scatter: null argument");
    if (columns < 1 || rfn < 1 || rfn > nr::kB2Waves || fh < 1 || fw < 1 || (long long)(rfn + 1) * fh * fw > 0x7fffffffLL)
        return fail("neuray_points_backward_scatter: bad shape");
    nr::ScatterSortedParams p;
    p.keys = sorted_keys_dev; p.perm = perm_dev; p.g = rows_dev; p.wts = rows_dev + 68; p.mask = nullptr;
    p.out0 = d_ray_feats_nhwc_dev; p.out1 = d_img_feats_nhwc_dev;
    p.m = columns * 4; p.img_stride = (long long)fh * fw * 32; p.tex_stride = 32; p.ch_stride = 1;
    p.ntex = rfn * fh * fw; p.hw = fh * fw; p.c = 64; p.split = 32; p.g_stride = nr::kB2ScatterRow; p.w_stride = nr::kB2ScatterRow;
    return scatter_sorted(p, stream);
#endif
}

int neuray_interpolate_scatter_keys(const float* points, const float* mask, int b, int n, int fh, int fw, int h_full, int w_full,
                                    int align_corners, int* keys_dev, float* wts_dev, void* stream) {
    if (!points || !keys_dev || !wts_dev) return fail("neuray_interpolate_scatter_keys: null argument");
    if (b < 1 || n < 1 || fh < 1 || fw < 1 || (long long)(b + 1) * fh * fw > 0x7fffffffLL) return fail("neuray_interpolate_scatter_keys: bad shape");
    NR_LAUNCH(nr::interpolate_scatter_keys_kernel, dim3(grid_for((long long)b * n, 256, 4096)), dim3(256), 0, stream, points, mask, b, n, fh,
              fw, h_full, w_full, align_corners, keys_dev, wts_dev);
    return check_launch("neuray_interpolate_scatter_keys");
}

int neuray_interpolate_feats_backward_sorted(const float* d_out, const float* mask, const int* sorted_keys_dev, const long long* perm_dev,
                                             const float* wts_dev, int b, int n, int c, int fh, int fw, float* d_feats, void* stream) {
    if (!d_out || !sorted_keys_dev || !perm_dev || !wts_dev || !d_feats) return fail("neuray_interpolate_feats_backward_sorted: null argument");
    if (b < 1 || n < 1 || c < 1 || fh < 1 || fw < 1 || (long long)(b + 1) * fh * fw > 0x7fffffffLL) return fail("neuray_interpolate_feats_backward_sorted: bad shape");
    nr::ScatterSortedParams p;
    p.keys = sorted_keys_dev; p.perm = perm_dev; p.g = d_out; p.wts = wts_dev; p.mask = mask; p.out0 = d_feats; p.out1 = d_feats;
    p.m = (long long)b * n * 4; p.img_stride = (long long)c * fh * fw; p.tex_stride = 1; p.ch_stride = (long long)fh * fw;
    p.ntex = b * fh * fw; p.hw = fh * fw; p.c = c; p.split = c; p.g_stride = c; p.w_stride = 4;
    return scatter_sorted(p, stream);
}

int neuray_inorm_chunks(int n, int c, int h, int w) {
    if (n < 1 || c < 1 || h < 1 || w < 1) return 0;
    return norm_chunks(n * c, h * w);
}

int neuray_group_sum_selftest(const float* x, float* y, void* stream) {
    NR_LAUNCH(nr::group_sum_selftest_kernel, dim3(1), dim3(64), 0, stream, x, y);
    return check_launch("neuray_group_sum_selftest");
}
int neuray_pair_forms_selftest(const float* x, float* y, void* stream) {
    NR_LAUNCH(nr::pair_forms_selftest_kernel, dim3(1), dim3(64), 0, stream, x, y);
    return check_launch("neuray_pair_forms_selftest");
}
int neuray_group_scatter_selftest(const float* x, float* y, void* stream) {
    NR_LAUNCH(nr::group_scatter_selftest_kernel, dim3(1), dim3(64), 0, stream, x, y);
    return check_launch("neuray_group_scatter_selftest");
}

// ---- image metrics (nr_kernels_metrics.h) -------------------------------------------------------------------------------------------
static void metrics_tiles(int y0, int y1, int x0, int x1, int& tiles_y, int& tiles_x) {
    tiles_y = (y1 - y0 - (nr::kMetWin - 1) + nr::kMetTH - 1) / nr::kMetTH;
    tiles_x = (x1 - x0 - (nr::kMetWin - 1) + nr::kMetTW - 1) / nr::kMetTW;
}

long long neuray_image_metrics_workspace_bytes(int n, int h, int w) {
    if (n < 1 || h < nr::kMetWin || w < nr::kMetWin) return -1;
    int ty, tx;
    metrics_tiles(0, h, 0, w, ty, tx);           // (a smaller ROI has fewer tiles)
    return (long long)n * ty * tx * nr::kMetPartial * 8;
}

int neuray_image_metrics(const NeurayImageMetricsArgs* a, void* stream) {
    if (!a) return fail("neuray_image_metrics: null args");
    if (!a->pred_dev || !a->gt_dev || !a->sse_dev || !a->ssim_dev || !a->workspace_dev) return fail("neuray_image_metrics: missing array");
    if (a->n < 1 || a->h < 1 || a->w < 1 || a->gt_stride < 0) return fail("neuray_image_metrics: bad shape n=%d h=%d w=%d gt_stride=%d", a->n, a->h, a->w, a->gt_stride);
    if (a->variant != NEURAY_SSIM_BOX11 && a->variant != NEURAY_SSIM_GAUSS11) return fail("neuray_image_metrics: unknown SSIM variant %d", a->variant);
    if (a->roi_y0 < 0 || a->roi_x0 < 0 || a->roi_y1 > a->h || a->roi_x1 > a->w || a->roi_y0 >= a->roi_y1 || a->roi_x0 >= a->roi_x1)
        return fail("neuray_image_metrics: region [%d, %d) x [%d, %d) is not inside the %d x %d image", a->roi_y0, a->roi_y1, a->roi_x0, a->roi_x1, a->h, a->w);
    if (a->roi_y1 - a->roi_y0 < nr::kMetWin || a->roi_x1 - a->roi_x0 < nr::kMetWin)
        return fail("neuray_image_metrics: the %d x %d region is smaller than the 11 x 11 SSIM window", a->roi_y1 - a->roi_y0, a->roi_x1 - a->roi_x0);
    nr::MetricsParams p;
    p.pred = a->pred_dev; p.gt = a->gt_dev; p.quant = a->quant_dev; p.sse = a->sse_dev; p.ssim = a->ssim_dev;
    p.ws = static_cast<double*>(a->workspace_dev);
    p.n = a->n; p.gt_stride = a->gt_stride; p.u8 = a->input_u8 ? 1 : 0; p.h = a->h; p.w = a->w;
    p.y0 = a->roi_y0; p.y1 = a->roi_y1; p.x0 = a->roi_x0; p.x1 = a->roi_x1;
    metrics_tiles(p.y0, p.y1, p.x0, p.x1, p.tiles_y, p.tiles_x);
    // tf.image.ssim's window (_fspecial_gauss: softmax of -0.5 (i^2 + j^2) / 1.5^2) is the outer product of this normalised 1-D one
    double sum = 0.0;
    for (int k = 0; k < nr::kMetWin; ++k) {
        const double d = k - (nr::kMetWin - 1) / 2;
        p.taps[k] = std::exp(-0.5 * d * d / (1.5 * 1.5));
        sum += p.taps[k];
    }
    for (int k = 0; k < nr::kMetWin; ++k) p.taps[k] /= sum;
    const long long blocks = (long long)p.n * p.tiles_y * p.tiles_x;
    if (blocks > 0x7fffffffLL) return fail("neuray_image_metrics: %lld tiles", blocks);
    const bool gauss = a->variant == NEURAY_SSIM_GAUSS11;
    auto k = gauss ? nr::image_metrics_tile_kernel<true> : nr::image_metrics_tile_kernel<false>;
    const size_t smem = gauss ? nr::metrics_smem_bytes<true>() : nr::metrics_smem_bytes<false>();     // 86 304 / 53 024 bytes
    launch_lds(k, dim3((unsigned)blocks), dim3(nr::kMetThreads), smem, stream, p);
    if (int rc = check_launch("neuray_image_metrics")) return rc;
    NR_LAUNCH(nr::image_metrics_reduce_kernel, dim3(p.n), dim3(64), 4 * 64 * 8, stream, p);
    return check_launch("neuray_image_metrics");
}

// ---- LPIPS (nr_kernels_lpips.h) -------------------------------------------------------------------------------------------------------
int neuray_lpips_stem(const void* img, int input_u8, const float* shift3, const float* scale3, const float* w, const float* bias, int n, int cout, int h, int wd,
                      float* out, void* stream) {
    if (!img || !shift3 || !scale3 || !w || !bias || !out) return fail("neuray_lpips_stem: null pointer");
    if (n < 1 || h < 1 || wd < 1 || cout < 1 || cout > nr::kLpStemMaxC) return fail("neuray_lpips_stem: bad shape n=%d cout=%d h=%d w=%d", n, cout, h, wd);
    const long long pixels = (long long)n * h * wd;
    if (pixels * cout * 4 >= 0x7fffff00LL) return fail("neuray_lpips_stem: the output must stay below 2^31 bytes");
    nr::LpipsStemParams p;
    p.img = img; p.wgt = w; p.bias = bias; p.out = out; p.n = n; p.cout = cout; p.h = h; p.w = wd; p.u8 = input_u8 ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
        if (!(scale3[c] != 0.0f)) return fail("neuray_lpips_stem: scale[%d] = %g", c, (double)scale3[c]);
        p.shift[c] = shift3[c]; p.scale[c] = scale3[c];
    }
    const size_t smem = (size_t)cout * 28 * sizeof(float);
    auto k = input_u8 ? nr::lpips_stem_kernel<true> : nr::lpips_stem_kernel<false>;
    NR_LAUNCH(k, dim3((unsigned)((pixels + nr::kLpThreads - 1) / nr::kLpThreads)), dim3(nr::kLpThreads), smem, stream, p);
    return check_launch("neuray_lpips_stem");
}

int neuray_maxpool2x2(const float* x, long long planes, int h, int w, float* out, void* stream) {
    if (!x || !out) return fail("neuray_maxpool2x2: null pointer");
    if (planes < 1 || h < 2 || w < 2) return fail("neuray_maxpool2x2: bad shape planes=%lld h=%d w=%d", planes, h, w);
    nr::MaxPoolParams p;
    p.x = x; p.out = out; p.h = h; p.w = w; p.total = planes * (h / 2) * (w / 2);
    const long long blocks = (p.total + nr::kLpThreads - 1) / nr::kLpThreads;
    if (blocks > 0x7fffffffLL) return fail("neuray_maxpool2x2: %lld elements", p.total);
    NR_LAUNCH(nr::maxpool2x2_kernel, dim3((unsigned)blocks), dim3(nr::kLpThreads), 0, stream, p);
    return check_launch("neuray_maxpool2x2");
}

long long neuray_lpips_head_workspace_bytes(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1) return -1;
    const long long tiles = ((long long)h * w + nr::kLpTile - 1) / nr::kLpTile;
    if (tiles * n > 0x7fffffffLL) return -1;
    return tiles * n * (long long)sizeof(double);
}

int neuray_lpips_head(const float* f0, const float* f1, const float* lin, int n, int f1_stride, int c, int h, int w, void* workspace, double* out,
                      int out_stride, void* stream) {
    if (!f0 || !f1 || !lin || !workspace || !out) return fail("neuray_lpips_head: null pointer");
    if (neuray_lpips_head_workspace_bytes(n, h, w) < 0 || c < 1 || f1_stride < 0 || f1_stride > 1 || out_stride < 1)
        return fail("neuray_lpips_head: bad shape n=%d c=%d h=%d w=%d f1_stride=%d out_stride=%d", n, c, h, w, f1_stride, out_stride);
    nr::LpipsHeadParams p;
    p.f0 = f0; p.f1 = f1; p.lin = lin; p.ws = static_cast<double*>(workspace); p.out = out;
    p.n = n; p.f1_stride = f1_stride; p.c = c; p.out_stride = out_stride; p.plane = (long long)h * w;
    p.tiles = (int)((p.plane + nr::kLpTile - 1) / nr::kLpTile);
    NR_LAUNCH(nr::lpips_head_tile_kernel, dim3((unsigned)(p.tiles * n)), dim3(nr::kLpThreads), 0, stream, p);
    if (int rc = check_launch("neuray_lpips_head")) return rc;
    NR_LAUNCH(nr::lpips_head_reduce_kernel, dim3((unsigned)n), dim3(64), 0, stream, p);
    return check_launch("neuray_lpips_head");
}

// ---- training losses (nr_kernels_loss.h) --------------------------------------------------------------------------------------------
// term table of the ABI -> the kernels' (chunks, first workgroup and first row of every term); 0 or the error already recorded
static int loss_params(const char* what, const NeurayLossTerm* terms, int n_terms, bool backward, nr::LossParams& p, long long& blocks) {
    if (!terms) return fail("%s: null term table", what);
    if (n_terms < 1 || n_terms > nr::kLossMaxTerms) return fail("%s: %d terms (1 .. %d)", what, n_terms, nr::kLossMaxTerms);
    blocks = 0;
    int rows = 0;
    for (int i = 0; i < n_terms; ++i) {
        const NeurayLossTerm& a = terms[i];
        nr::LossTerm& t = p.t[i];
        if (a.kind != NEURAY_LOSS_RENDER && a.kind != NEURAY_LOSS_CONSIST && a.kind != NEURAY_LOSS_DEPTH) return fail("%s: term %d: unknown kind %d", what, i, a.kind);
        if (!a.pred_dev || !a.ref_dev) return fail("%s: term %d: missing array", what, i);
        if (a.rows < 1) return fail("%s: term %d: %d rows", what, i, a.rows);
        if (a.n < 1 || a.n > (1 << 30)) return fail("%s: term %d: %d elements per row", what, i, a.n);
        if (a.kind == NEURAY_LOSS_CONSIST && (a.inner < 1 || a.n % a.inner != 0)) return fail("%s: term %d: n=%d is not rn * dn with dn=%d", what, i, a.n, a.inner);
        if (a.kind == NEURAY_LOSS_DEPTH) {
            if (!a.coords_dev || !a.range_dev) return fail("%s: term %d: missing array", what, i);
            if (a.h < 2 || a.w < 2) return fail("%s: term %d: the depth gather needs a map of at least 2 x 2 (h=%d w=%d)", what, i, a.h, a.w);
            if ((long long)a.h * a.w > 0x7fffffffLL) return fail("%s: term %d: map %d x %d", what, i, a.h, a.w);
            if (a.stride < 1) return fail("%s: term %d: element stride %d", what, i, a.stride);
            if (a.smooth_l1 && !(a.beta >= 0.0f)) return fail("%s: term %d: beta %g", what, i, (double)a.beta);
        }
        if (backward && a.d_pred_dev && !a.grad_out_dev) return fail("%s: term %d: missing upstream gradient", what, i);
        t.pred = a.pred_dev; t.ref = a.ref_dev; t.mask = a.kind == NEURAY_LOSS_CONSIST ? nullptr : a.mask_dev;
        t.coords = a.coords_dev; t.range = a.range_dev; t.g_up = a.grad_out_dev; t.d_pred = a.d_pred_dev;
        t.kind = a.kind; t.rows = a.rows; t.n = a.n; t.inner = a.kind == NEURAY_LOSS_CONSIST ? a.inner : 1;
        t.stride = a.kind == NEURAY_LOSS_DEPTH ? a.stride : 1; t.h = a.h; t.w = a.w; t.coords_i64 = a.coords_i64 ? 1 : 0;
        t.mask_u8 = a.kind == NEURAY_LOSS_RENDER && a.mask_u8 ? 1 : 0; t.smooth_l1 = a.smooth_l1 ? 1 : 0;
        t.beta = a.beta; t.thresh = a.thresh;
        t.chunks = (a.n + nr::kLossChunk - 1) / nr::kLossChunk;
        if (blocks + (long long)t.chunks * a.rows > 0x7fffffffLL || rows > 0x7fffffff - a.rows) return fail("%s: too many rows", what);
        t.block0 = (int)blocks; t.row0 = rows;
        blocks += (long long)t.chunks * a.rows;
        rows += a.rows;
    }
    p.nterms = n_terms; p.total_rows = rows;
    return 0;
}

long long neuray_train_loss_workspace_bytes(const NeurayLossTerm* terms, int n_terms) {
    nr::LossParams p = {};
    long long blocks;
    if (loss_params("neuray_train_loss_workspace_bytes", terms, n_terms, false, p, blocks)) return -1;
    return blocks * 2 * (long long)sizeof(double);
}

int neuray_train_loss(const NeurayTrainLossArgs* a, void* stream) {
    if (!a) return fail("neuray_train_loss: null args");
    nr::LossParams p = {};
    long long blocks;
    if (int rc = loss_params("neuray_train_loss", a->terms, a->n_terms, false, p, blocks)) return rc;
    if (!a->value_dev || !a->den_dev || !a->workspace_dev) return fail("neuray_train_loss: missing array");
    p.ws = static_cast<double*>(a->workspace_dev); p.value = a->value_dev; p.den = a->den_dev;
    NR_LAUNCH(nr::loss_partials_kernel, dim3((unsigned)blocks), dim3(nr::kLossThreads), 2 * nr::kLossThreads * sizeof(double), stream, p);
    if (int rc = check_launch("neuray_train_loss")) return rc;
    NR_LAUNCH(nr::loss_finish_kernel, dim3((unsigned)p.total_rows), dim3(64), 2 * 64 * sizeof(double), stream, p);
    return check_launch("neuray_train_loss");
}

int neuray_train_loss_backward(const NeurayTrainLossArgs* a, void* stream) {
    if (!a) return fail("neuray_train_loss_backward: null args");
    nr::LossParams p = {};
    long long blocks;
    if (int rc = loss_params("neuray_train_loss_backward", a->terms, a->n_terms, true, p, blocks)) return rc;
    if (!a->den_dev) return fail("neuray_train_loss_backward: missing array");
    p.ws = nullptr; p.value = nullptr; p.den = a->den_dev;
    NR_LAUNCH(nr::loss_backward_kernel, dim3((unsigned)blocks), dim3(nr::kLossThreads), 0, stream, p);
    return check_launch("neuray_train_loss_backward");
}

int neuray_visibility_points(const NeurayVisibilityArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_visibility_points: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_visibility_points: null args");
    if (a->rfn < 1 || a->rfn > NEURAY_MAX_VIEWS) return fail("neuray_visibility_points: rfn=%d outside [1,%d]", a->rfn, NEURAY_MAX_VIEWS);
    if (a->dn <= 2 || a->dn > NEURAY_MAX_SAMPLES || a->rn < 1) return fail("neuray_visibility_points: bad rn=%d dn=%d (dn in [3,%d])", a->rn, a->dn, NEURAY_MAX_SAMPLES);
    if (a->h < 2 || a->w < 2 || a->fh < 1 || a->fw < 1) return fail("neuray_visibility_points: bad shape h=%d w=%d fh=%d fw=%d", a->h, a->w, a->fh, a->fw);
    if (a->use_vis && !a->has_vis_head) return fail("neuray_visibility_points: use_vis set but the decoder has no vis head");
    if ((long long)a->rn * a->dn > 0x7fffffffLL / 2) return fail("neuray_visibility_points: rn*dn too large for one call");
    if ((long long)a->rfn * a->fh * a->fw * 128 >= 0x7fffff00LL) return fail("neuray_visibility_points: the ray_feats maps must stay below 2^31 bytes");
    if (!a->query_const_dev || !a->view_const_dev || !a->coords_dev || !a->depth_dev || !a->ray_feats_nhwc_dev || !a->packed_weights_dev)
        return fail("neuray_visibility_points: missing input array");
    if (!a->alpha_dev || !a->nvalid_dev) return fail("neuray_visibility_points: alpha_dev / nvalid_dev missing");
    nr::VisParams p;
    p.que_const = a->query_const_dev; p.view_const = a->view_const_dev; p.coords = a->coords_dev; p.depth = a->depth_dev;
    p.ray_feats = a->ray_feats_nhwc_dev; p.weights = a->packed_weights_dev; p.alpha = a->alpha_dev; p.nvalid = a->nvalid_dev;
    p.rfn = a->rfn; p.rn = a->rn; p.dn = a->dn; p.h = a->h; p.w = a->w; p.fh = a->fh; p.fw = a->fw;
    p.use_vis = a->use_vis; p.var_bias = a->var_bias; p.ground = a->ground;
    const int nwaves = (a->rfn + 1) / 2;
    const long long tiles = (long long)((a->rn + 15) / 16) * a->dn;
    int grid = grid_for(tiles, 1, NR_POINT_GRID);         // the point kernel's persistent-style grid
    if (tiles >= 4096 && grid > tiles / NR_POINT_MIN_TILES) grid = (int)(tiles / NR_POINT_MIN_TILES);
    grid = (grid + 7) / 8 * 8;                             // (the XCD-aware tile map needs a multiple of 8)
    const size_t smem = nr::vis_smem_bytes();
    // the vis head is evaluated only when compute_prob consumes it (as neuray_render_points)
    if (a->has_vis_head && a->use_vis) NR_LAUNCH(nr::vis_points_kernel<true>, dim3(grid), dim3(64 * nwaves), smem, stream, p);
    else NR_LAUNCH(nr::vis_points_kernel<false>, dim3(grid), dim3(64 * nwaves), smem, stream, p);
    return check_launch("neuray_visibility_points");
#endif
}

int neuray_visibility_rays(const float* alpha, const int* nvalid, int rn, int dn, int view_num, int point_num, float* hit_prob,
                           unsigned char* ray_mask, void* stream) {
#ifdef NR_BF16_QUADS
    (void)alpha; (void)nvalid; (void)rn; (void)dn; (void)view_num; (void)point_num; (void)hit_prob; (void)ray_mask; (void)stream;
    return fail("neuray_visibility_rays: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (rn < 1 || dn < 1 || dn > NEURAY_MAX_SAMPLES) return fail("neuray_visibility_rays: bad shape rn=%d dn=%d", rn, dn);
    if (!alpha || !nvalid || !hit_prob) return fail("neuray_visibility_rays: alpha / nvalid / hit_prob missing");
    const int grid = grid_for(rn, 64, 256 * 8);
    NR_LAUNCH(nr::vis_rays_kernel, dim3(grid), dim3(64), 0, stream, alpha, nvalid, rn, dn, view_num, point_num, hit_prob, ray_mask);
    return check_launch("neuray_visibility_rays");
#endif
}

int neuray_procedural_render(const NeurayProceduralArgs* a, void* stream) {
    if (!a) return fail("neuray_procedural_render: null args");
    if (a->ss < 1 || a->ss > 4) return fail("neuray_procedural_render: ss=%d outside [1,4]", a->ss);
    if (a->n_prims < 0 || a->n_prims > NEURAY_PROC_MAX_PRIMS) return fail("neuray_procedural_render: n_prims=%d outside [0,%d]", a->n_prims, NEURAY_PROC_MAX_PRIMS);
    if (a->n < 1 || a->h < 1 || a->w < 1) return fail("neuray_procedural_render: bad size n=%d h=%d w=%d", a->n, a->h, a->w);
    if (a->n > 65535 || (a->h + nr::kProcTileY - 1) / nr::kProcTileY > 65535) return fail("neuray_procedural_render: n=%d h=%d too large for one call", a->n, a->h);
    if (!a->scene_dev || !a->poses_dev || !a->Ks_inv_dev || !a->rgb_dev) return fail("neuray_procedural_render: scene / poses / Ks_inv / rgb missing");
    nr::ProcParams p;
    p.scene = a->scene_dev; p.poses = a->poses_dev; p.Ks_inv = a->Ks_inv_dev;
    p.rgb = a->rgb_dev; p.depth = a->depth_dev; p.mask = a->mask_dev; p.prim = a->prim_dev;
    p.n_prims = a->n_prims; p.n = a->n; p.h = a->h; p.w = a->w; p.ss = a->ss;
    const dim3 grid((unsigned)((a->w + nr::kProcTileX - 1) / nr::kProcTileX), (unsigned)((a->h + nr::kProcTileY - 1) / nr::kProcTileY), (unsigned)a->n);
    NR_LAUNCH(nr::procedural_render_kernel, grid, dim3(nr::kProcTileX * nr::kProcTileY), 0, stream, p);
    return check_launch("neuray_procedural_render");
}

// ---- augmentation of the procedural stream ----
#ifndef NR_BF16_QUADS
static_assert(NEURAY_AUGMENT_STATS == nr::kAugStats && NEURAY_AUGMENT_PLAN == nr::kAugPlan && NEURAY_AUGMENT_HOST == nr::kAugHost, "abi");
static_assert(NEURAY_SAMPLE_COORDS_WORK == nr::kSampleWorkWords, "abi");
static int augment_common(const char* who, int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1) return fail("%s: bad size n=%d h=%d w=%d", who, n, h, w);
    if (n > 65535) return fail("%s: n=%d too large for one call", who, n);
    if ((long long)h * w > 0x7fffffffLL) return fail("%s: h*w too large (a pixel index is an int)", who);
    return 0;
}
#endif

int neuray_augment_stats(const NeurayAugmentStatsArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_augment_stats: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_augment_stats: null args");
    if (int rc = augment_common("neuray_augment_stats", a->n, a->h, a->w)) return rc;
    if (!a->mask_dev || !a->depth_dev || !a->row_counts_dev || !a->row_part_dev || !a->stats_dev) return fail("neuray_augment_stats: mask / depth / row_counts / row_part / stats missing");
    nr::AugStatsParams p;
    p.mask = a->mask_dev; p.depth = a->depth_dev; p.row_counts = a->row_counts_dev; p.row_part = a->row_part_dev; p.stats = a->stats_dev;
    p.n = a->n; p.h = a->h; p.w = a->w;
    NR_LAUNCH(nr::augment_row_stats_kernel, dim3((unsigned)a->h, (unsigned)a->n), dim3(nr::kAugBlock), 0, stream, p);
    NR_LAUNCH(nr::augment_view_stats_kernel, dim3((unsigned)a->n), dim3(nr::kAugBlock), 0, stream, p);
    return check_launch("neuray_augment_stats");
#endif
}

int neuray_augment_depth(const NeurayAugmentDepthArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_augment_depth: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_augment_depth: null args");
    if (int rc = augment_common("neuray_augment_depth", a->n, a->h, a->w)) return rc;
    if (a->rfn < 0 || a->view0 < 0 || a->view0 + a->rfn > a->n) return fail("neuray_augment_depth: working views [%d,%d) outside [0,%d)", a->view0, a->view0 + a->rfn, a->n);
    if (!a->depth_dev || !a->mask_dev || !a->range_in_dev || !a->stats_dev || !a->row_counts_dev || !a->host_dev) return fail("neuray_augment_depth: depth / mask / range_in / stats / row_counts / host missing");
    if (!a->range_aug_dev || !a->range_out_dev || (a->rfn > 0 && (!a->plan_dev || !a->depth_aug_dev))) return fail("neuray_augment_depth: range_aug / range_out / plan / depth_aug missing");
    nr::AugDepthParams p;
    p.depth = a->depth_dev; p.mask = a->mask_dev; p.range_in = a->range_in_dev; p.stats = a->stats_dev; p.row_counts = a->row_counts_dev;
    p.host = a->host_dev; p.range_aug = a->range_aug_dev; p.range_out = a->range_out_dev; p.plan = a->plan_dev; p.depth_aug = a->depth_aug_dev;
    p.n = a->n; p.h = a->h; p.w = a->w; p.view0 = a->view0; p.rfn = a->rfn; p.key0 = a->key0; p.key1 = a->key1;
    NR_LAUNCH(nr::augment_plan_kernel, dim3((unsigned)(a->rfn > 0 ? a->rfn : 1)), dim3(64), 0, stream, p);
    if (a->rfn > 0) {
        const long long plane = (long long)a->h * a->w;
        NR_LAUNCH(nr::augment_apply_kernel, dim3((unsigned)((plane + nr::kAugBlock - 1) / nr::kAugBlock), (unsigned)a->rfn), dim3(nr::kAugBlock), 0, stream, p);
    }
    return check_launch("neuray_augment_depth");
#endif
}

int neuray_sample_coords(const NeuraySampleCoordsArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_sample_coords: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_sample_coords: null args");
    if (int rc = augment_common("neuray_sample_coords", 1, a->h, a->w)) return rc;
    const long long N = (long long)a->h * a->w;
    if (a->ray_num < 1 || a->ray_num > N) return fail("neuray_sample_coords: ray_num=%d outside [1, h*w=%lld]", a->ray_num, N);
    if (a->want_fg < 0 || a->want_fg > a->ray_num) return fail("neuray_sample_coords: want_fg=%d outside [0, ray_num=%d]", a->want_fg, a->ray_num);
    if (!a->mask_dev || !a->keys_dev || !a->taken_dev || !a->work_dev || !a->coords_dev) return fail("neuray_sample_coords: mask / keys / taken / work / coords missing");
    nr::SampleParams p;
    p.mask = a->mask_dev; p.keys = a->keys_dev; p.taken = a->taken_dev; p.work = a->work_dev; p.coords = a->coords_dev;
    p.N = (int)N; p.w = a->w; p.ray_num = a->ray_num; p.want_fg = a->want_fg; p.view = a->view; p.key0 = a->key0; p.key1 = a->key1;
    // every workgroup owns `chunk` consecutive pixels (a multiple of 256, at least 1024), at most kSampleMaxBlocks workgroups
    long long chunk = (N + nr::kSampleMaxBlocks - 1) / nr::kSampleMaxBlocks;
    chunk = (chunk + nr::kAugBlock - 1) / nr::kAugBlock * nr::kAugBlock;
    if (chunk < 4 * nr::kAugBlock) chunk = 4 * nr::kAugBlock;
    p.chunk = (int)chunk; p.nblocks = (int)((N + chunk - 1) / chunk);
    p.stage = 0; p.pass = 0;
    const dim3 grid((unsigned)p.nblocks), block(nr::kAugBlock);
    NR_LAUNCH(nr::sample_keys_kernel, grid, block, 0, stream, p);
    for (int stage = 0; stage < 2; ++stage) {
        p.stage = stage;
        for (int pass = 0; pass < nr::kSamplePasses; ++pass) {
            p.pass = pass;
            NR_LAUNCH(nr::sample_hist_kernel, grid, block, 0, stream, p);
        }
        NR_LAUNCH(nr::sample_count_kernel, grid, block, 0, stream, p);
        NR_LAUNCH(nr::sample_emit_kernel, grid, block, 0, stream, p);
    }
    return check_launch("neuray_sample_coords");
#endif
}

// ---- geometry export ----
#ifndef NR_BF16_QUADS
static int fuse_common(const char* who, const void* depth, const void* poses, const void* Ks, const void* Ks_inv, const void* nn_ids, int n, int h,
                       int w, int n_src) {
    if (n < 1 || h < 1 || w < 1) return fail("%s: bad size n=%d h=%d w=%d", who, n, h, w);
    if (n_src < 1 || n_src > NEURAY_FUSE_MAX_SRC) return fail("%s: n_src=%d outside [1,%d]", who, n_src, NEURAY_FUSE_MAX_SRC);
    if (n > 65535 || (h + nr::kFuseTileY - 1) / nr::kFuseTileY > 65535) return fail("%s: n=%d h=%d too large for one call", who, n, h);
    if ((long long)h * w > 0x7fffffffLL) return fail("%s: h*w too large (a texel index is an int)", who);
    if (!depth || !poses || !Ks || !Ks_inv || !nn_ids) return fail("%s: depth / poses / Ks / Ks_inv / nn_ids missing", who);
    return 0;
}
#endif

int neuray_depth_consistency(const NeurayDepthConsistencyArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_depth_consistency: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_depth_consistency: null args");
    if (int rc = fuse_common("neuray_depth_consistency", a->depth_dev, a->poses_dev, a->Ks_dev, a->Ks_inv_dev, a->nn_ids_dev, a->n, a->h, a->w, a->n_src)) return rc;
    if (!(a->tau_px > 0.0f) || !(a->tau_d > 0.0f)) return fail("neuray_depth_consistency: thresholds must be positive (tau_px=%g tau_d=%g)", a->tau_px, a->tau_d);
    nr::FuseConsistencyParams p;
    p.depth = a->depth_dev; p.poses = a->poses_dev; p.Ks = a->Ks_dev; p.Ks_inv = a->Ks_inv_dev; p.nn_ids = a->nn_ids_dev;
    p.count = a->count_dev; p.fused_depth = a->fused_depth_dev; p.consistent_bits = a->consistent_bits_dev; p.occluded_bits = a->occluded_bits_dev;
    p.src_texel = a->src_texel_dev;
    p.n = a->n; p.h = a->h; p.w = a->w; p.S = a->n_src; p.tau_px = a->tau_px; p.tau_d = a->tau_d;
    const dim3 grid((unsigned)((a->w + nr::kFuseTileX - 1) / nr::kFuseTileX), (unsigned)((a->h + nr::kFuseTileY - 1) / nr::kFuseTileY), (unsigned)a->n);
    NR_LAUNCH(nr::depth_consistency_kernel, grid, dim3(nr::kFuseTileX * nr::kFuseTileY), 0, stream, p);
    return check_launch("neuray_depth_consistency");
#endif
}

int neuray_fuse_view(const NeurayFuseViewArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_fuse_view: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_fuse_view: null args");
    if (int rc = fuse_common("neuray_fuse_view", a->depth_dev, a->poses_dev, a->Ks_dev, a->Ks_inv_dev, a->nn_ids_dev, a->n, a->h, a->w, a->n_src)) return rc;
    if (a->view < 0 || a->view >= a->n) return fail("neuray_fuse_view: view=%d outside [0,%d)", a->view, a->n);
    if (a->min_views < 1) return fail("neuray_fuse_view: min_views=%d (at least 1)", a->min_views);
    if (!(a->tau_n > 0.0f)) return fail("neuray_fuse_view: thresholds must be positive (tau_n=%g)", a->tau_n);
    if (!a->count_dev || !a->fused_depth_dev || !a->consistent_bits_dev) return fail("neuray_fuse_view: count / fused_depth / consistent_bits missing");
    if (!a->emit_dev || !a->xyz_dev) return fail("neuray_fuse_view: emit / xyz missing");
    if (a->colour_dev && !a->rgb_dev) return fail("neuray_fuse_view: colour asked for without rgb");
    if (a->dedup && !a->taken_dev) return fail("neuray_fuse_view: dedup set but taken missing");
    nr::FuseParams p;
    p.depth = a->depth_dev; p.poses = a->poses_dev; p.Ks = a->Ks_dev; p.Ks_inv = a->Ks_inv_dev; p.nn_ids = a->nn_ids_dev;
    p.count = a->count_dev; p.fused_depth = a->fused_depth_dev; p.consistent_bits = a->consistent_bits_dev; p.rgb = a->rgb_dev;
    p.taken = a->dedup ? a->taken_dev : nullptr;
    p.emit = a->emit_dev; p.xyz = a->xyz_dev; p.colour = a->colour_dev; p.normal = a->normal_dev;
    p.n = a->n; p.h = a->h; p.w = a->w; p.S = a->n_src; p.view = a->view; p.min_views = a->min_views; p.tau_n = a->tau_n;
    const dim3 grid((unsigned)((a->w + nr::kFuseTileX - 1) / nr::kFuseTileX), (unsigned)((a->h + nr::kFuseTileY - 1) / nr::kFuseTileY), 1u);
    NR_LAUNCH(nr::fuse_view_kernel, grid, dim3(nr::kFuseTileX * nr::kFuseTileY), 0, stream, p);
    return check_launch("neuray_fuse_view");
#endif
}

// ---- mesh export ----
#ifndef NR_BF16_QUADS
// the lattice of a volume: every dimension >= 2, at most 2^30 points
static int tsdf_dims(const char* who, int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return fail("%s: bad dims nx=%d ny=%d nz=%d (each at least 2)", who, nx, ny, nz);
    if ((long long)nx * ny * nz > (1LL << 30)) return fail("%s: nx*ny*nz=%lld lattice points (at most 2^30)", who, (long long)nx * ny * nz);
    return 0;
}
// the tiles per row (bx) and per slice (by) of a box of (ex, ey, ez) elements -> the number of workgroups (bx * by * ez <= ex * ey * ez <= 2^30)
static unsigned tsdf_grid(int ex, int ey, int ez, int& bx, int& by) {
    bx = (ex + nr::kTsdfTileX - 1) / nr::kTsdfTileX; by = (ey + nr::kTsdfTileY - 1) / nr::kTsdfTileY;
    return (unsigned)((long long)bx * by * ez);
}
#endif

int neuray_tsdf_integrate(const NeurayTsdfIntegrateArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_tsdf_integrate: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_tsdf_integrate: null args");
    if (int rc = tsdf_dims("neuray_tsdf_integrate", a->nx, a->ny, a->nz)) return rc;
    if (a->n < 1 || a->h < 1 || a->w < 1) return fail("neuray_tsdf_integrate: bad size n=%d h=%d w=%d", a->n, a->h, a->w);
    if ((long long)a->h * a->w > 0x7fffffffLL) return fail("neuray_tsdf_integrate: h*w too large (a texel index is an int)");
    if (a->v0 < 0 || a->v1 > a->n || a->v0 > a->v1) return fail("neuray_tsdf_integrate: views [%d,%d) outside [0,%d)", a->v0, a->v1, a->n);
    if (!(a->voxel_size > 0.0f) || !(a->trunc > 0.0f)) return fail("neuray_tsdf_integrate: voxel_size and trunc must be positive (voxel_size=%g trunc=%g)", a->voxel_size, a->trunc);
    if (!a->depth_dev || !a->poses_dev || !a->Ks_dev || !a->tsum_dev || !a->w_dev) return fail("neuray_tsdf_integrate: depth / poses / Ks / tsum / w missing");
    const int colour = (a->rgb_dev != nullptr) + (a->csum_dev != nullptr) + (a->cw_dev != nullptr);
    if (colour != 0 && colour != 3) return fail("neuray_tsdf_integrate: rgb, csum and cw go together (all or none)");
    if (a->v0 == a->v1) return 0;
    nr::TsdfIntegrateParams p;
    p.depth = a->depth_dev; p.rgb = a->rgb_dev; p.poses = a->poses_dev; p.Ks = a->Ks_dev;
    p.tsum = a->tsum_dev; p.wsum = a->w_dev; p.csum = a->csum_dev; p.cw = a->cw_dev;
    p.ox = a->origin_x; p.oy = a->origin_y; p.oz = a->origin_z; p.vs = a->voxel_size; p.trunc = a->trunc;
    p.nx = a->nx; p.ny = a->ny; p.nz = a->nz; p.h = a->h; p.w = a->w; p.v0 = a->v0; p.v1 = a->v1;
    const unsigned blocks = tsdf_grid(a->nx, a->ny, a->nz, p.bx, p.by);
    NR_LAUNCH(nr::tsdf_integrate_kernel, dim3(blocks), dim3(nr::kTsdfTileX * nr::kTsdfTileY), 0, stream, p);
    return check_launch("neuray_tsdf_integrate");
#endif
}

int neuray_surface_cells(const NeuraySurfaceCellsArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_surface_cells: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_surface_cells: null args");
    if (int rc = tsdf_dims("neuray_surface_cells", a->nx, a->ny, a->nz)) return rc;
    if (!(a->min_weight > 0.0f)) return fail("neuray_surface_cells: min_weight=%g must be positive", a->min_weight);
    if (!a->tsum_dev || !a->w_dev || !a->cells_dev) return fail("neuray_surface_cells: tsum / w / cells missing");
    nr::SurfaceCellsParams p;
    p.tsum = a->tsum_dev; p.wsum = a->w_dev; p.cells = a->cells_dev; p.nx = a->nx; p.ny = a->ny; p.nz = a->nz; p.min_weight = a->min_weight;
    const unsigned blocks = tsdf_grid(a->nx - 1, a->ny - 1, a->nz - 1, p.bx, p.by);
    NR_LAUNCH(nr::surface_cells_kernel, dim3(blocks), dim3(nr::kTsdfTileX * nr::kTsdfTileY), 0, stream, p);
    return check_launch("neuray_surface_cells");
#endif
}

int neuray_surface_emit(const NeuraySurfaceEmitArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_surface_emit: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_surface_emit: null args");
    if (int rc = tsdf_dims("neuray_surface_emit", a->nx, a->ny, a->nz)) return rc;
    if (!(a->voxel_size > 0.0f)) return fail("neuray_surface_emit: voxel_size=%g must be positive", a->voxel_size);
    if (a->n_vertices > (1u << 30) || a->n_quads > 3u * (1u << 30)) return fail("neuray_surface_emit: bad totals n_vertices=%u n_quads=%u", a->n_vertices, a->n_quads);
    if (!a->tsum_dev || !a->w_dev || !a->cells_dev || !a->vert_offset_dev || !a->quad_offset_dev) return fail("neuray_surface_emit: tsum / w / cells / offsets missing");
    if ((a->csum_dev != nullptr) != (a->cw_dev != nullptr)) return fail("neuray_surface_emit: csum and cw go together");
    if (a->n_vertices == 0) return 0;
    if (!a->vertices_dev || !a->normals_dev || !a->colours_dev || (a->n_quads > 0 && !a->faces_dev)) return fail("neuray_surface_emit: vertices / normals / colours / faces missing");
    nr::SurfaceEmitParams p;
    p.tsum = a->tsum_dev; p.wsum = a->w_dev; p.csum = a->csum_dev; p.cw = a->cw_dev; p.cells = a->cells_dev;
    p.vert_offset = a->vert_offset_dev; p.quad_offset = a->quad_offset_dev;
    p.vertices = a->vertices_dev; p.normals = a->normals_dev; p.colours = a->colours_dev; p.faces = a->faces_dev;
    p.n_vertices = a->n_vertices; p.n_quads = a->n_quads;
    p.ox = a->origin_x; p.oy = a->origin_y; p.oz = a->origin_z; p.vs = a->voxel_size; p.nx = a->nx; p.ny = a->ny; p.nz = a->nz;
    const unsigned blocks = tsdf_grid(a->nx - 1, a->ny - 1, a->nz - 1, p.bx, p.by);
    NR_LAUNCH(nr::surface_emit_kernel, dim3(blocks), dim3(nr::kTsdfTileX * nr::kTsdfTileY), 0, stream, p);
    return check_launch("neuray_surface_emit");
#endif
}

// ---- ray casting of a volume ----
int neuray_surface_blocks(const NeuraySurfaceBlocksArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_surface_blocks: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_surface_blocks: null args");
    if (int rc = tsdf_dims("neuray_surface_blocks", a->nx, a->ny, a->nz)) return rc;
    if (!a->cells_dev || !a->blocks_dev) return fail("neuray_surface_blocks: cells / blocks missing");
    nr::SurfaceBlocksParams p;
    p.cells = a->cells_dev; p.blocks = a->blocks_dev; p.mx = a->nx - 1; p.my = a->ny - 1; p.mz = a->nz - 1;
    p.bx = (p.mx + nr::kTsdfBlock - 1) / nr::kTsdfBlock; p.by = (p.my + nr::kTsdfBlock - 1) / nr::kTsdfBlock;
    const int bz = (p.mz + nr::kTsdfBlock - 1) / nr::kTsdfBlock;
    NR_LAUNCH(nr::surface_blocks_kernel, dim3((unsigned)(p.bx * p.by * bz)), dim3(64), 0, stream, p);          // (at most 2^21 blocks)
    return check_launch("neuray_surface_blocks");
#endif
}

int neuray_tsdf_raycast(const NeurayTsdfRaycastArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_tsdf_raycast: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_tsdf_raycast: null args");
    if (int rc = tsdf_dims("neuray_tsdf_raycast", a->nx, a->ny, a->nz)) return rc;
    if (a->n < 1 || a->n > 65535 || a->h < 1 || a->w < 1) return fail("neuray_tsdf_raycast: bad size n=%d h=%d w=%d (n in 1 .. 65535, h and w positive)", a->n, a->h, a->w);
    if ((long long)a->h * a->w > 0x7fffffffLL) return fail("neuray_tsdf_raycast: h*w too large (a pixel index is an int)");
    if (!(a->voxel_size > 0.0f)) return fail("neuray_tsdf_raycast: voxel_size=%g must be positive", a->voxel_size);
    if (!(a->step > 0.0f) || !(a->step <= 0.95f)) return fail("neuray_tsdf_raycast: step=%g outside (0, 0.95] voxels", a->step);
    if (!a->field_dev || !a->rays_dev || !a->depth_dev || !a->status_dev) return fail("neuray_tsdf_raycast: field / rays / depth / status missing");
    if ((a->csum_dev != nullptr) != (a->cw_dev != nullptr)) return fail("neuray_tsdf_raycast: csum and cw go together");
    nr::TsdfRaycastParams p;
    p.field = a->field_dev; p.csum = a->csum_dev; p.cw = a->cw_dev; p.rays = a->rays_dev; p.range = a->depth_range_dev; p.blocks = a->blocks_dev;
    p.depth = a->depth_dev; p.normal = a->normal_dev; p.colours = a->colours_dev; p.status = a->status_dev; p.evaluated = a->evaluated_dev;
    p.ox = a->origin_x; p.oy = a->origin_y; p.oz = a->origin_z; p.vs = a->voxel_size; p.step = a->step;
    p.nx = a->nx; p.ny = a->ny; p.nz = a->nz; p.h = a->h; p.w = a->w;
    p.bx = (a->nx - 1 + nr::kTsdfBlock - 1) / nr::kTsdfBlock; p.by = (a->ny - 1 + nr::kTsdfBlock - 1) / nr::kTsdfBlock;
    const dim3 grid((unsigned)((a->w + nr::kRaycastTileX - 1) / nr::kRaycastTileX), (unsigned)((a->h + nr::kRaycastTileY - 1) / nr::kRaycastTileY), (unsigned)a->n);
    if (grid.y > 65535u) return fail("neuray_tsdf_raycast: h=%d too large (at most %d)", a->h, 65535 * nr::kRaycastTileY);
    NR_LAUNCH(nr::tsdf_raycast_kernel, grid, dim3(nr::kRaycastTileX * nr::kRaycastTileY), 0, stream, p);
    return check_launch("neuray_tsdf_raycast");
#endif
}

// ---- plane-sweep stereo ----
#ifndef NR_BF16_QUADS
extern "C++" {
template <int R>
static void launch_plane_sweep(const nr::SweepParams& p, dim3 grid, void* stream) {
    // the smallest costs kept per plane: ceil(S / 2) of them enter the mean
    if (p.S <= 4) NR_LAUNCH((nr::plane_sweep_kernel<R, 2>), grid, dim3(nr::kSweepThreads), 0, stream, p);
    else if (p.S <= 8) NR_LAUNCH((nr::plane_sweep_kernel<R, 4>), grid, dim3(nr::kSweepThreads), 0, stream, p);
    else NR_LAUNCH((nr::plane_sweep_kernel<R, 8>), grid, dim3(nr::kSweepThreads), 0, stream, p);
}
}  // extern "C++"
#endif

int neuray_plane_sweep(const NeurayPlaneSweepArgs* a, void* stream) {
#ifdef NR_BF16_QUADS
    (void)a; (void)stream;
    return fail("neuray_plane_sweep: lives in the fp32 library (this is a bf16-operand variant build)");
#else
    if (!a) return fail("neuray_plane_sweep: null args");
    if (a->radius < 1 || a->radius > nr::kSweepMaxRadius) return fail("neuray_plane_sweep: radius=%d outside [1,%d]", a->radius, nr::kSweepMaxRadius);
    if (a->n < 1 || a->h < 2 * a->radius + 1 || a->w < 2 * a->radius + 1) return fail("neuray_plane_sweep: bad size n=%d h=%d w=%d (radius %d)", a->n, a->h, a->w, a->radius);
    if (a->n_src < 1 || a->n_src > nr::kSweepMaxSrc) return fail("neuray_plane_sweep: n_src=%d outside [1,%d]", a->n_src, nr::kSweepMaxSrc);
    if (a->planes < 3 || a->planes > NEURAY_SWEEP_MAX_PLANES) return fail("neuray_plane_sweep: planes=%d outside [3,%d]", a->planes, NEURAY_SWEEP_MAX_PLANES);
    if (a->v0 < 0 || a->v1 <= a->v0 || a->v1 > a->n) return fail("neuray_plane_sweep: views [%d,%d) of %d", a->v0, a->v1, a->n);
    if (a->min_src < 0 || !(a->var_min > 0.0f)) return fail("neuray_plane_sweep: min_src=%d var_min=%g", a->min_src, a->var_min);
    if ((long long)a->h * a->w > 0x7fffffffLL || (long long)a->n * a->n_src > 0x7ffffffLL) return fail("neuray_plane_sweep: h*w or n*n_src too large");
    const unsigned gx = (unsigned)((a->w + nr::kSweepTile - 1) / nr::kSweepTile), gy = (unsigned)((a->h + nr::kSweepTile - 1) / nr::kSweepTile);
    if (a->v1 - a->v0 > 65535 || gy > 65535u) return fail("neuray_plane_sweep: %d views of height %d are too many for one call", a->v1 - a->v0, a->h);
    if (!a->imgs_dev || !a->gray_dev || !a->cams_dev || !a->depth_range_dev || !a->nn_ids_dev) return fail("neuray_plane_sweep: imgs / gray / cams / depth_range / nn_ids missing");
    if (!a->depth_dev || !a->cost_dev || !a->plane_dev) return fail("neuray_plane_sweep: depth / cost / plane missing");
    nr::SweepParams p;
    p.rgb = a->imgs_dev; p.gray = a->gray_dev; p.cams = a->cams_dev; p.range = a->depth_range_dev; p.nn_ids = a->nn_ids_dev;
    p.depth = a->depth_dev; p.cost = a->cost_dev; p.plane = a->plane_dev;
    p.n = a->n; p.h = a->h; p.w = a->w; p.S = a->n_src; p.D = a->planes; p.v0 = a->v0; p.v1 = a->v1; p.min_src = a->min_src; p.flags = a->flags;
    p.var_min = a->var_min;
    NR_LAUNCH(nr::sweep_gray_kernel, dim3((unsigned)grid_for((long long)a->n * a->h * a->w, 256, 65536)), dim3(256), 0, stream, p);
    const dim3 grid(gx, gy, (unsigned)(a->v1 - a->v0));
    if (a->radius == 1) launch_plane_sweep<1>(p, grid, stream);
    else if (a->radius == 2) launch_plane_sweep<2>(p, grid, stream);
    else launch_plane_sweep<3>(p, grid, stream);
    return check_launch("neuray_plane_sweep");
#endif
}

#ifdef NR_B2_PROFILE
// profile build only (tools/profile_bwd2.py): read (and optionally clear) the per-mark cycle sums of points_backward2_kernel
int neuray_debug_b2_profile(unsigned long long* out, int clear) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(nr::nr_b2_prof), sizeof(unsigned long long) * nr::kB2Marks * 8) != hipSuccess) return 1;
    if (clear) {
        static unsigned long long zeros[nr::kB2Marks * 8] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(nr::nr_b2_prof), zeros, sizeof(zeros)) != hipSuccess) return 1;
    }
    return 0;
}
#endif

}  // extern "C"
