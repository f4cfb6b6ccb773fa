// ppp_api.hip -- the extern "C" entry points declared in include/ppp_mi355x.h.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "ppp_kernels.hpp"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(PPP_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// largest float <= t  /  smallest float >= t
float round_down_f32(double t) {
    float f = (float)t;
    if ((double)f > t) f = std::nextafterf(f, -INFINITY);
    return f;
}
float round_up_f32(double t) {
    float f = (float)t;
    if ((double)f < t) f = std::nextafterf(f, INFINITY);
    return f;
}

int make_geo(const ppp_params *p, ppp::Geo *G) {
    if (!p) return fail(PPP_ERR_INVALID_ARG, "params is NULL");
    if (p->abi_version != PPP_ABI_VERSION)
        return fail(PPP_ERR_INVALID_ARG, "abi_version %d != %d", p->abi_version, PPP_ABI_VERSION);
    if (p->Z <= 0 || p->Y <= 0 || p->X <= 0)
        return fail(PPP_ERR_INVALID_ARG, "bad volume %d x %d x %d", p->Z, p->Y, p->X);
    if (p->pz <= 0 || p->py <= 0 || p->px <= 0 || !(p->pz & 1) || !(p->py & 1) || !(p->px & 1))
        return fail(PPP_ERR_INVALID_ARG, "patch shape must be positive and odd (%d,%d,%d)", p->pz,
                    p->py, p->px);
    if (!(p->th > 0.0 && p->th < 1.0)) return fail(PPP_ERR_INVALID_ARG, "th must be in (0,1)");
    if ((long long)p->Z * p->Y * p->X >= (1ll << 31))
        return fail(PPP_ERR_UNSUPPORTED, "volumes of 2^31 voxels or more are not supported");
    ppp::Geo g;
    memset(&g, 0, sizeof(g));
    g.Z = p->Z; g.Y = p->Y; g.X = p->X;
    g.pz = p->pz; g.py = p->py; g.px = p->px;
    g.rz = p->pz / 2; g.ry = p->py / 2; g.rx = p->px / 2;
    g.C = p->pz * p->py * p->px;
    g.mid = g.C / 2;
    g.V = (long long)p->Z * p->Y * p->X;
    g.th_gt = round_down_f32(p->th);
    double bg;
    switch (p->bg_rule) {
    case PPP_BG_INV_TH: bg = p->thi; break;
    case PPP_BG_HALF_TH: bg = p->th / 2; break;
    case PPP_BG_LESS_THAN_TH: bg = p->th; break;
    default: return fail(PPP_ERR_INVALID_ARG, "how is bg defined for vote instances? (bg_rule %d)", p->bg_rule);
    }
    g.bg_lt = round_up_f32(bg);
    g.th_rn = (float)p->th;
    g.th2 = p->th * p->th;
    g.den = 1.0 - p->th * p->th;
    if (p->value_rule < PPP_VAL_COUNT || p->value_rule > PPP_VAL_NORM_PROB_PRODUCT)
        return fail(PPP_ERR_INVALID_ARG, "bad value_rule %d", p->value_rule);
    g.value_rule = p->value_rule;
    g.use_overlap = p->use_overlap != 0;
    g.normalise = p->normalise != 0;
    g.norm_rank = p->norm_rank != 0;
    g.count_pos_neg = p->count_pos_neg != 0;
    g.norm_aff = p->norm_aff != 0;
    g.layout = p->cons_layout;
    const ppp_box &b = p->cons_box;
    if (b.z0 < 0 || b.y0 < 0 || b.x0 < 0 || b.z1 > p->Z || b.y1 > p->Y || b.x1 > p->X ||
        b.z1 <= b.z0 || b.y1 <= b.y0 || b.x1 <= b.x0)
        return fail(PPP_ERR_INVALID_ARG, "cons_box outside the volume or empty");
    if (g.layout == PPP_CONS_REFERENCE) {
        if (b.z0 || b.y0 || b.x0 || b.z1 != p->Z || b.y1 != p->Y || b.x1 != p->X)
            return fail(PPP_ERR_INVALID_ARG, "reference layout needs cons_box = whole volume");
    } else if (g.layout != PPP_CONS_COMPACT && g.layout != PPP_CONS_VOXEL_MAJOR) {
        return fail(PPP_ERR_INVALID_ARG, "bad cons_layout %d", p->cons_layout);
    }
    g.bz0 = b.z0; g.by0 = b.y0; g.bx0 = b.x0;
    g.bZ = b.z1 - b.z0; g.bY = b.y1 - b.y0; g.bX = b.x1 - b.x0;
    g.BV = (long long)g.bZ * g.bY * g.bX;
    g.cz0 = g.bz0; g.cy0 = g.by0; g.cx0 = g.bx0;
    g.cZ = g.bZ; g.cY = g.bY; g.cX = g.bX;
    g.nsy = 2 * p->py; g.nsx = 2 * p->px;
    g.wy = 2 * p->py - 1; g.wx = 2 * p->px - 1;
    g.n_planes = ((2 * p->pz - 1) * g.wy * g.wx - 1) / 2;
    g.oz = p->origin_z; g.oy = p->origin_y; g.ox = p->origin_x;
    if (p->ring_z < 0 || (p->ring_z > 0 && (g.layout != PPP_CONS_VOXEL_MAJOR || g.bZ > p->ring_z || p->origin_z < 0)))
        return fail(PPP_ERR_INVALID_ARG, "ring_z: VOXEL_MAJOR rows only, cons_box at most ring_z slices thick");
    g.ring = p->ring_z;
    g.pred_clean = p->pred_clean == 1 ? 1 : 0;
    if (p->rank_tile < 0 || p->rank_tile > 3) return fail(PPP_ERR_INVALID_ARG, "rank_tile must be 0 .. 3");
    g.rank_tile = p->rank_tile;
    *G = g;
    return PPP_OK;
}

int need_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(PPP_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    return PPP_OK;
}

int check_dtype(int dt) {
    if (dt != PPP_F32 && dt != PPP_F16 && dt != PPP_BF16) return fail(PPP_ERR_INVALID_ARG, "bad pred dtype %d", dt);
    return PPP_OK;
}
// the entry points that write a prediction, or exist for benches and profiles only
int check_dtype_f32_f16(int dt, const char *who) {
    if (dt == PPP_BF16)
        return fail(PPP_ERR_INVALID_ARG, "%s: pred dtype %d (bfloat16) is not supported here, float32 / float16 only", who, dt);
    return check_dtype(dt);
}

}  // namespace

#define PPP_TRY(expr)            \
    do {                         \
        int rc_ = (expr);        \
        if (rc_ != PPP_OK) return rc_; \
    } while (0)

namespace ppp {
static int g_env_epoch = 0;
int env_epoch() { return g_env_epoch; }
void env_reload() { ++g_env_epoch; }
}  // namespace ppp

extern "C" {

int ppp_abi_version(void) { return PPP_ABI_VERSION; }
const char *ppp_last_error(void) { return g_err; }
const char *ppp_consensus_kernel_name(void) { return ppp::last_consensus_kernel(); }
int ppp_consensus_short_form(void) { return ppp::last_consensus_short_form(); }
const char *ppp_rank_kernel_name(void) { return ppp::last_rank_kernel(); }
const char *ppp_patch_graph_kernel_name(void) { return ppp::last_patch_graph_kernel(); }
const char *ppp_patch_graph_kernel_geometry(void) { return ppp::last_patch_graph_geometry(); }

void ppp_reload_env(void) { ppp::env_reload(); }

int ppp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ppp_pred_dtype_supported(int dtype) { return check_dtype(dtype) == PPP_OK ? 1 : 0; }

int64_t ppp_cons_planes(const ppp_params *p) {
    if (!p) return -1;
    if (p->cons_layout == PPP_CONS_REFERENCE)
        return (int64_t)(p->pz > 1 ? 2 * p->pz : p->pz) * (2 * p->py) * (2 * p->px);
    const int64_t w = (int64_t)(2 * p->pz - 1) * (2 * p->py - 1) * (2 * p->px - 1);
    return p->cons_layout == PPP_CONS_VOXEL_MAJOR ? w : (w - 1) / 2;
}

int64_t ppp_cons_elems(const ppp_params *p) {
    if (!p) return -1;
    const ppp_box &b = p->cons_box;
    return ppp_cons_planes(p) * (int64_t)(b.z1 - b.z0) * (b.y1 - b.y0) * (b.x1 - b.x0);
}

int ppp_consensus(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, float *d_cons,
                  float *d_count, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || (!d_cons && !d_count)) return fail(PPP_ERR_INVALID_ARG, "NULL pred / outputs");
    if (G.use_overlap && !d_overlap) return fail(PPP_ERR_INVALID_ARG, "use_overlap set but d_overlap is NULL");
    if (G.layout == PPP_CONS_VOXEL_MAJOR && (!ppp::consensus_v3_supported(G) || d_count || !d_cons))
        return fail(PPP_ERR_UNSUPPORTED, "ppp_consensus writes VOXEL_MAJOR only with the packed kernel (TH = 0.5, normalised "
                                         "product, px in {3,5,7,9}; no counts): see ppp_consensus_writes_voxel_major");
    if (G.ring) return fail(PPP_ERR_UNSUPPORTED, "ring_z: rows of a ring are written by ppp_consensus_part");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_consensus(d_pred, pred_dtype, d_overlap, d_cons, d_count, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_consensus");
}

int ppp_consensus_rows(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, float *d_cons,
                       const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || !d_cons) return fail(PPP_ERR_INVALID_ARG, "NULL pred / outputs");
    if (G.use_overlap && !d_overlap) return fail(PPP_ERR_INVALID_ARG, "use_overlap set but d_overlap is NULL");
    if (G.layout != PPP_CONS_VOXEL_MAJOR || !ppp::consensus_v3_supported(G))
        return fail(PPP_ERR_UNSUPPORTED, "ppp_consensus_rows writes VOXEL_MAJOR rows with the packed kernel only "
                                         "(see ppp_consensus_writes_voxel_major)");
    if (G.ring) return fail(PPP_ERR_UNSUPPORTED, "ring_z: rows of a ring are written by ppp_consensus_part");
    PPP_TRY(need_device());
    G.vm_open = 1;
    hipError_t e = ppp::launch_consensus(d_pred, pred_dtype, d_overlap, d_cons, nullptr, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_consensus_rows");
}

int ppp_consensus_part(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, float *d_cons,
                       const ppp_params *p, const ppp_box *part, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || !d_cons || !part) return fail(PPP_ERR_INVALID_ARG, "NULL pred / output / part");
    if (G.use_overlap && !d_overlap) return fail(PPP_ERR_INVALID_ARG, "use_overlap set but d_overlap is NULL");
    if ((G.layout != PPP_CONS_VOXEL_MAJOR && G.layout != PPP_CONS_COMPACT) || !ppp::consensus_v3_supported(G))
        return fail(PPP_ERR_UNSUPPORTED, "ppp_consensus_part writes COMPACT planes or VOXEL_MAJOR rows with the packed "
                                         "kernel only (see ppp_consensus_writes_voxel_major)");
    const ppp_box &b = p->cons_box;
    if (part->z0 < b.z0 || part->y0 < b.y0 || part->x0 < b.x0 || part->z1 > b.z1 || part->y1 > b.y1 ||
        part->x1 > b.x1 || part->z1 <= part->z0 || part->y1 <= part->y0 || part->x1 <= part->x0)
        return fail(PPP_ERR_INVALID_ARG, "part must be a non-empty sub-box of cons_box");
    PPP_TRY(need_device());
    G.vm_open = 1;
    G.cz0 = part->z0; G.cy0 = part->y0; G.cx0 = part->x0;
    G.cZ = part->z1 - part->z0; G.cY = part->y1 - part->y0; G.cX = part->x1 - part->x0;
    hipError_t e = ppp::launch_consensus_part(d_pred, pred_dtype, d_overlap, d_cons, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_consensus_part");
}

// ---- S1 on sparse foreground: the item pre-pass and the launch over item lists ----
static long long g_s1_items = 0, g_s1_active = 0;
static int g_s1_took_lists = 0;

// the Geo of a sparse call (NULL part: the whole cons_box); what ppp_consensus_part checks of `part`
static int sparse_geo(const ppp_params *p, const ppp_box *part, ppp::Geo *G) {
    PPP_TRY(make_geo(p, G));
    if (!part) return PPP_OK;
    const ppp_box &b = p->cons_box;
    if (part->z0 < b.z0 || part->y0 < b.y0 || part->x0 < b.x0 || part->z1 > b.z1 || part->y1 > b.y1 ||
        part->x1 > b.x1 || part->z1 <= part->z0 || part->y1 <= part->y0 || part->x1 <= part->x0)
        return fail(PPP_ERR_INVALID_ARG, "part must be a non-empty sub-box of cons_box");
    G->cz0 = part->z0; G->cy0 = part->y0; G->cx0 = part->x0;
    G->cZ = part->z1 - part->z0; G->cY = part->y1 - part->y0; G->cX = part->x1 - part->x0;
    return PPP_OK;
}

int64_t ppp_consensus_sparse_workspace_bytes(const ppp_params *p, const ppp_box *part) {
    ppp::Geo G;
    if (!p || sparse_geo(p, part, &G) != PPP_OK) return 0;
    return (int64_t)ppp::consensus_sparse_workspace_bytes(G);
}

int ppp_consensus_sparse(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, float *d_cons,
                         float *d_count, const ppp_params *p, const ppp_box *part, int open_rows, void *d_work,
                         int mode, void *stream) {
    ppp::Geo G;
    PPP_TRY(sparse_geo(p, part, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || (!d_cons && !d_count) || (part && !d_cons)) return fail(PPP_ERR_INVALID_ARG, "NULL pred / outputs");
    if (part && d_count) return fail(PPP_ERR_INVALID_ARG, "a part writes no counts (as ppp_consensus_part)");
    if (G.use_overlap && !d_overlap) return fail(PPP_ERR_INVALID_ARG, "use_overlap set but d_overlap is NULL");
    if (mode != 0 && mode != 1) return fail(PPP_ERR_INVALID_ARG, "mode must be 0 (auto) or 1 (lists)");
    if ((G.layout != PPP_CONS_VOXEL_MAJOR && G.layout != PPP_CONS_COMPACT) || !ppp::consensus_v3_supported(G) ||
        (G.layout == PPP_CONS_VOXEL_MAJOR && (d_count || !d_cons)))
        return fail(PPP_ERR_UNSUPPORTED, "ppp_consensus_sparse serves the packed kernel only: COMPACT planes (with counts) "
                                         "or VOXEL_MAJOR rows (see ppp_consensus_writes_voxel_major)");
    if (G.ring && !part) return fail(PPP_ERR_UNSUPPORTED, "ring_z: rows of a ring are written part by part");
    if (ppp::consensus_sparse_workspace_bytes(G) == 0)
        return fail(PPP_ERR_UNSUPPORTED, "ppp_consensus_sparse: too many work items for 32-bit item numbers");
    if (!d_work) return fail(PPP_ERR_INVALID_ARG, "d_work is NULL (ppp_consensus_sparse_workspace_bytes)");
    PPP_TRY(need_device());
    if (part || open_rows) G.vm_open = 1;
    hipError_t e = ppp::run_consensus_sparse(d_pred, pred_dtype, d_overlap, d_cons, d_count, G, d_work, mode, &g_s1_items,
                                             &g_s1_active, &g_s1_took_lists, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_consensus_sparse");
}

void ppp_consensus_last_items(int64_t *total, int64_t *active, int *took_lists) {
    if (total) *total = g_s1_items;
    if (active) *active = g_s1_active;
    if (took_lists) *took_lists = g_s1_took_lists;
}

int ppp_consensus_writes_voxel_major(const ppp_params *p) {
    ppp::Geo G;
    if (!p || make_geo(p, &G) != PPP_OK) return 0;
    return ppp::consensus_v3_supported(G) ? 1 : 0;
}

int ppp_rank_patches(const void *d_pred, int pred_dtype, const float *d_cons,
                     const uint8_t *d_overlap, float *d_score, const ppp_box *score_box,
                     const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || !d_cons || !d_score) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.use_overlap && !d_overlap) return fail(PPP_ERR_INVALID_ARG, "use_overlap set but d_overlap is NULL");
    if (G.layout == PPP_CONS_VOXEL_MAJOR) return fail(PPP_ERR_UNSUPPORTED, "ppp_rank_patches reads COMPACT or REFERENCE layout");
    ppp_box sb = {0, 0, 0, p->Z, p->Y, p->X};
    if (score_box) sb = *score_box;
    if (sb.z0 < 0 || sb.y0 < 0 || sb.x0 < 0 || sb.z1 > p->Z || sb.y1 > p->Y || sb.x1 > p->X)
        return fail(PPP_ERR_INVALID_ARG, "score_box outside the volume");
    // the consensus tile must hold every base voxel the scored centres read
    if (!ppp::cons_box_covers(G, sb))
        return fail(PPP_ERR_INVALID_ARG, "cons_box does not cover score_box grown by the patch radius");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_rank(d_pred, pred_dtype, d_cons, d_overlap, d_score, sb, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_rank_patches");
}

static int rank_box(const ppp_box *score_box, const ppp_params *p, const ppp::Geo &G, ppp_box *sb) {
    *sb = ppp_box{0, 0, 0, p->Z, p->Y, p->X};
    if (score_box) *sb = *score_box;
    if (sb->z0 < 0 || sb->y0 < 0 || sb->x0 < 0 || sb->z1 > p->Z || sb->y1 > p->Y || sb->x1 > p->X ||
        sb->z1 <= sb->z0 || sb->y1 <= sb->y0 || sb->x1 <= sb->x0)
        return fail(PPP_ERR_INVALID_ARG, "score_box outside the volume");
    if (!ppp::cons_box_covers(G, *sb))
        return fail(PPP_ERR_INVALID_ARG, "cons_box does not cover score_box grown by the patch radius");
    return PPP_OK;
}

int64_t ppp_rank_workspace_bytes(const ppp_box *score_box, const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    if (!ppp::rank_vm_supported(G)) return 0;
    // (rows in a ring: the workgroup-per-tile kernel only -- a caller planning a ring asks with ring_z set)
    if (G.ring && !ppp::rank_wg_supported(G)) return 0;
    ppp_box sb;
    if (rank_box(score_box, p, G, &sb) != PPP_OK) return -1;
    return (int64_t)ppp::rank_vm_workspace_bytes(sb, G);
}

int ppp_rank_wg_plan(const ppp_box *score_box, const ppp_params *p, int resident_per_cu, int cus_per_xcd, int32_t *plan) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (!plan) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (!ppp::rank_wg_supported(G))
        return fail(PPP_ERR_UNSUPPORTED, "ppp_rank_wg_plan: the workgroup-per-tile kernel does not serve these parameters");
    ppp_box sb;
    PPP_TRY(rank_box(score_box, p, G, &sb));
    if (resident_per_cu <= 0 || cus_per_xcd <= 0) PPP_TRY(need_device());
    ppp::rank_wg_plan(sb, G, resident_per_cu, cus_per_xcd, plan);
    return PPP_OK;
}

int ppp_rank_wg_plan_residency(const ppp_box *score_box, const ppp_params *p, int resident_per_cu, int cus_per_xcd, int32_t *res) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (!res) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (!ppp::rank_wg_supported(G))
        return fail(PPP_ERR_UNSUPPORTED, "ppp_rank_wg_plan_residency: the workgroup-per-tile kernel does not serve these parameters");
    ppp_box sb;
    PPP_TRY(rank_box(score_box, p, G, &sb));
    if (resident_per_cu <= 0 || cus_per_xcd <= 0) PPP_TRY(need_device());
    ppp::rank_wg_plan_residency(sb, G, resident_per_cu, cus_per_xcd, res);
    return PPP_OK;
}

#ifdef PPP_RW_STAMPS
// diagnostic build only, not in the header: where ppp_rank_patches_vm's workspace holds the stamps (-1: nowhere)
extern "C" int64_t ppp_rank_wg_stamps_offset(const ppp_box *score_box, const ppp_params *p) {
    ppp::Geo G;
    ppp_box sb;
    if (make_geo(p, &G) != PPP_OK || !ppp::rank_wg_supported(G) || rank_box(score_box, p, G, &sb) != PPP_OK) return -1;
    return (int64_t)ppp::rank_wg_stamps_offset(sb, G);
}
#endif

int ppp_rank_patches_vm(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                        const uint8_t *d_overlap, float *d_score, const ppp_box *score_box,
                        void *d_work, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || !d_cons_vm || !d_score || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.use_overlap && !d_overlap) return fail(PPP_ERR_INVALID_ARG, "use_overlap set but d_overlap is NULL");
    if (!ppp::rank_vm_supported(G))
        return fail(PPP_ERR_UNSUPPORTED, "ppp_rank_patches_vm: VOXEL_MAJOR layout, cubic patches of 3/5/7/9, "
                                         "no count_pos_neg (use ppp_rank_patches otherwise)");
    if (G.ring && !ppp::rank_wg_supported(G))
        return fail(PPP_ERR_UNSUPPORTED, "ring_z: only the workgroup-per-tile ranking kernel reads a ring of rows");
    ppp_box sb;
    PPP_TRY(rank_box(score_box, p, G, &sb));
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_rank_vm(d_pred, pred_dtype, d_cons_vm, d_overlap, d_score, sb, d_work, G,
                                       (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_rank_patches_vm");
}

// the *_slices entry points: the z axis is a stack of independent 2-d images (pz = 1)
static int slices_geo(const ppp_params *p, int slices, ppp::Geo *G) {
    PPP_TRY(make_geo(p, G));
    if (slices) {
        if (G->pz != 1) return fail(PPP_ERR_INVALID_ARG, "independent slices need 2-d patches (pz = 1, not %d)", G->pz);
        G->slice_seeds = 1;
    }
    return PPP_OK;
}

static int patch_graph_impl(const void *d_pred, int pred_dtype, const float *d_cons,
                            const uint32_t *d_pairs, const uint32_t *d_order, uint64_t n_pairs,
                            float *d_aff, const ppp_params *p, void *stream, int slices) {
    ppp::Geo G;
    PPP_TRY(slices_geo(p, slices, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (n_pairs == 0) return PPP_OK;
    if (n_pairs >= (1ull << 32)) return fail(PPP_ERR_UNSUPPORTED, "more than 2^32-1 pair rows");
    if (!d_pred || !d_cons || !d_pairs || !d_aff) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.ring) return fail(PPP_ERR_UNSUPPORTED, "ring_z: only ppp_patch_graph_by_patch reads a ring of rows");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_patch_graph(d_pred, pred_dtype, d_cons, d_pairs, d_order, n_pairs, d_aff, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_graph");
}

int ppp_patch_graph(const void *d_pred, int pred_dtype, const float *d_cons,
                    const uint32_t *d_pairs, const uint32_t *d_order, uint64_t n_pairs,
                    float *d_aff, const ppp_params *p, void *stream) {
    return patch_graph_impl(d_pred, pred_dtype, d_cons, d_pairs, d_order, n_pairs, d_aff, p, stream, 0);
}

int ppp_patch_graph_slices(const void *d_pred, int pred_dtype, const float *d_cons,
                           const uint32_t *d_pairs, const uint32_t *d_order, uint64_t n_pairs,
                           float *d_aff, const ppp_params *p, void *stream) {
    return patch_graph_impl(d_pred, pred_dtype, d_cons, d_pairs, d_order, n_pairs, d_aff, p, stream, 1);
}

int32_t ppp_patch_graph_by_patch_chunk(const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    return ppp::patch_graph_pa_chunk(G, false);
}

int32_t ppp_patch_graph_by_patch_chunk_small(const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    return ppp::patch_graph_pa_chunk(G, true);
}

int64_t ppp_patch_graph_lcg_words(int32_t dz, int32_t dy, int32_t dx, const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return 0;
    return ppp::patch_graph_lcg_words(G, dz, dy, dx);
}

int ppp_patch_plane_bits(const uint32_t *words, int32_t n_words, int32_t px, uint64_t *planes) {
    if (!words || !planes) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (px != 3 && px != 5 && px != 7 && px != 9)
        return fail(PPP_ERR_UNSUPPORTED, "ppp_patch_plane_bits: px %d (plane values are kept for px in {3, 5, 7, 9})", px);
    if (n_words != (px * px * px + 31) / 32)
        return fail(PPP_ERR_INVALID_ARG, "ppp_patch_plane_bits: %d words for a %d^3 patch", n_words, px);
    const int rpc = 64 / px < px ? 64 / px : px;          // rows of a plane's first chunk (9^3: 7 of 9)
    for (int z = 0; z < px; ++z) {
        planes[z] = ppp::patch_plane_bits(words, n_words, z * px * px, rpc * px);
        if (rpc < px) planes[px + z] = ppp::patch_plane_bits(words, n_words, (z * px + rpc) * px, (px - rpc) * px);
    }
    return PPP_OK;
}

static int patch_graph_lcg_impl(const void *d_pred, int pred_dtype, const uint32_t *d_pairs,
                                const uint32_t *d_order, const int64_t *d_lcg_pos, int64_t n_lcg,
                                const int64_t *d_drop_off, uint64_t *d_drops, const ppp_params *p,
                                void *stream, int slices) {
    ppp::Geo G;
    PPP_TRY(slices_geo(p, slices, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (n_lcg <= 0) return PPP_OK;
    if (!d_pred || !d_pairs || !d_order || !d_lcg_pos || !d_drop_off || !d_drops)
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_patch_graph_lcg(d_pred, pred_dtype, d_pairs, d_order, (const long long *)d_lcg_pos,
                                               (long long)n_lcg, (const long long *)d_drop_off,
                                               (unsigned long long *)d_drops, G, (hipStream_t)stream);
    if (e == hipErrorNotSupported)
        return fail(PPP_ERR_UNSUPPORTED, "no per-patch kernel for this patch shape");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_graph_lcg");
}

int ppp_patch_graph_lcg(const void *d_pred, int pred_dtype, const uint32_t *d_pairs,
                        const uint32_t *d_order, const int64_t *d_lcg_pos, int64_t n_lcg,
                        const int64_t *d_drop_off, uint64_t *d_drops, const ppp_params *p, void *stream) {
    return patch_graph_lcg_impl(d_pred, pred_dtype, d_pairs, d_order, d_lcg_pos, n_lcg, d_drop_off, d_drops,
                                p, stream, 0);
}

int ppp_patch_graph_lcg_slices(const void *d_pred, int pred_dtype, const uint32_t *d_pairs,
                               const uint32_t *d_order, const int64_t *d_lcg_pos, int64_t n_lcg,
                               const int64_t *d_drop_off, uint64_t *d_drops, const ppp_params *p,
                               void *stream) {
    return patch_graph_lcg_impl(d_pred, pred_dtype, d_pairs, d_order, d_lcg_pos, n_lcg, d_drop_off, d_drops,
                                p, stream, 1);
}

int ppp_patch_graph_by_patch_chunked(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                                     const uint32_t *d_pairs, const uint32_t *d_order,
                                     const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                                     int32_t n_groups, int64_t n_blocks, int32_t chunk, float *d_aff,
                                     const ppp_params *p, void *stream) {
    return ppp_patch_graph_by_patch_lcg(d_pred, pred_dtype, d_cons_vm, d_pairs, d_order, d_group_start,
                                        d_chunk_offsets, n_groups, n_blocks, chunk, d_aff, nullptr, nullptr,
                                        p, stream);
}

static int patch_graph_by_patch_impl(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                                     const uint32_t *d_pairs, const uint32_t *d_order,
                                     const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                                     int32_t n_groups, int64_t n_blocks, int32_t chunk, float *d_aff,
                                     const int64_t *d_drop_off, const uint64_t *d_drops,
                                     const int64_t *d_bits_centres, int64_t n_bits, const uint32_t *d_bits,
                                     const ppp_params *p, void *stream, int slices) {
    ppp::Geo G;
    PPP_TRY(slices_geo(p, slices, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (n_groups == 0) return PPP_OK;
    if (!d_pred || !d_cons_vm || !d_pairs || !d_order || !d_group_start || !d_chunk_offsets || !d_aff)
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.layout != PPP_CONS_VOXEL_MAJOR)
        return fail(PPP_ERR_INVALID_ARG, "ppp_patch_graph_by_patch reads the VOXEL_MAJOR layout");
    if ((d_drop_off == nullptr) != (d_drops == nullptr))
        return fail(PPP_ERR_INVALID_ARG, "d_drop_off and d_drops go together");
    if (d_bits && (!d_bits_centres || n_bits <= 0 || n_bits >= (1ll << 31)))
        return fail(PPP_ERR_INVALID_ARG, "d_bits needs its sorted centre list");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_patch_graph_pa(d_pred, pred_dtype, d_cons_vm, d_pairs, d_order,
                                              (const long long *)d_group_start,
                                              (const long long *)d_chunk_offsets, n_groups, n_blocks,
                                              chunk, d_aff, (const long long *)d_drop_off,
                                              (const unsigned long long *)d_drops,
                                              d_bits ? (const long long *)d_bits_centres : nullptr,
                                              d_bits ? (int)n_bits : 0, d_bits, G, (hipStream_t)stream);
    if (e == hipErrorNotSupported)
        return fail(PPP_ERR_UNSUPPORTED, "no per-patch kernel for this patch shape / chunk size");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_graph_by_patch");
}

int ppp_patch_graph_by_patch_lcg(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                                 const uint32_t *d_pairs, const uint32_t *d_order,
                                 const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                                 int32_t n_groups, int64_t n_blocks, int32_t chunk, float *d_aff,
                                 const int64_t *d_drop_off, const uint64_t *d_drops,
                                 const ppp_params *p, void *stream) {
    return patch_graph_by_patch_impl(d_pred, pred_dtype, d_cons_vm, d_pairs, d_order, d_group_start,
                                     d_chunk_offsets, n_groups, n_blocks, chunk, d_aff, d_drop_off, d_drops,
                                     nullptr, 0, nullptr, p, stream, 0);
}

int ppp_patch_graph_by_patch_bits(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                                  const uint32_t *d_pairs, const uint32_t *d_order,
                                  const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                                  int32_t n_groups, int64_t n_blocks, int32_t chunk, float *d_aff,
                                  const int64_t *d_drop_off, const uint64_t *d_drops,
                                  const int64_t *d_bits_centres, int64_t n_bits, const uint32_t *d_bits,
                                  int32_t slices, const ppp_params *p, void *stream) {
    return patch_graph_by_patch_impl(d_pred, pred_dtype, d_cons_vm, d_pairs, d_order, d_group_start,
                                     d_chunk_offsets, n_groups, n_blocks, chunk, d_aff, d_drop_off, d_drops,
                                     d_bits_centres, n_bits, d_bits, p, stream, slices ? 1 : 0);
}

int ppp_patch_fg_bits(const void *d_pred, int pred_dtype, const int64_t *d_centres, int64_t n,
                      uint32_t *d_bits, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (n <= 0) return PPP_OK;
    if (!d_pred || !d_centres || !d_bits) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_patch_fg_bits(d_pred, pred_dtype, (const long long *)d_centres, (long long)n,
                                             d_bits, G, (hipStream_t)stream);
    if (e == hipErrorNotSupported) return fail(PPP_ERR_UNSUPPORTED, "too many centres for one launch");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_fg_bits");
}

int ppp_patch_graph_by_patch_lcg_slices(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                                        const uint32_t *d_pairs, const uint32_t *d_order,
                                        const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                                        int32_t n_groups, int64_t n_blocks, int32_t chunk, float *d_aff,
                                        const int64_t *d_drop_off, const uint64_t *d_drops,
                                        const ppp_params *p, void *stream) {
    return patch_graph_by_patch_impl(d_pred, pred_dtype, d_cons_vm, d_pairs, d_order, d_group_start,
                                     d_chunk_offsets, n_groups, n_blocks, chunk, d_aff, d_drop_off, d_drops,
                                     nullptr, 0, nullptr, p, stream, 1);
}

int ppp_patch_graph_by_patch(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                             const uint32_t *d_pairs, const uint32_t *d_order,
                             const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                             int32_t n_groups, int64_t n_blocks, float *d_aff,
                             const ppp_params *p, void *stream) {
    return ppp_patch_graph_by_patch_chunked(d_pred, pred_dtype, d_cons_vm, d_pairs, d_order, d_group_start,
                                            d_chunk_offsets, n_groups, n_blocks,
                                            ppp_patch_graph_by_patch_chunk(p), d_aff, p, stream);
}

size_t ppp_label_workspace_bytes(const ppp_params *p) {
    if (!p) return 0;
    return (size_t)24 * (size_t)p->Z * p->Y * p->X;
}

int ppp_label_begin(const uint32_t *d_nodes, uint64_t n_nodes, void *d_work, const ppp_params *p,
                    void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n_nodes == 0) return PPP_OK;
    if (!d_nodes || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.V >= (1ll << 32)) return fail(PPP_ERR_UNSUPPORTED, "more than 2^32-1 voxels");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_label_begin(d_nodes, n_nodes, d_work, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_label_begin");
}

int ppp_label_add(const uint32_t *d_pairs, const float *d_aff, const int64_t *d_row_ids,
                  int64_t first_row_id, uint64_t n_pairs, void *d_work, const ppp_params *p,
                  void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n_pairs == 0) return PPP_OK;
    if (!d_pairs || !d_aff || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_label_add(d_pairs, d_aff, (const long long *)d_row_ids,
                                         (long long)first_row_id, n_pairs, d_work, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_label_add");
}

int ppp_label_union_edges(const int64_t *d_a, const int64_t *d_b, uint64_t n, void *d_work,
                          const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n == 0) return PPP_OK;
    if (!d_a || !d_b || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_label_union_edges((const long long *)d_a, (const long long *)d_b, n,
                                                 d_work, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_label_union_edges");
}

int ppp_label_finish(const uint32_t *d_nodes, uint64_t n_nodes, int64_t *d_node_key, void *d_work,
                     const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n_nodes == 0) return PPP_OK;
    if (!d_nodes || !d_node_key || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_label_finish(d_nodes, n_nodes, (long long *)d_node_key, nullptr,
                                            d_work, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_label_finish");
}

int ppp_label_components(const uint32_t *d_pairs, const float *d_aff, uint64_t n_pairs,
                         const uint32_t *d_nodes, uint64_t n_nodes, uint32_t *d_node_key,
                         void *d_work, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n_nodes == 0) return PPP_OK;
    if (n_pairs >= (1ull << 31)) return fail(PPP_ERR_UNSUPPORTED, "more than 2^31-1 pair rows");
    if ((n_pairs && (!d_pairs || !d_aff)) || !d_nodes || !d_node_key || !d_work)
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_label(d_pairs, d_aff, n_pairs, d_nodes, n_nodes, d_node_key, d_work, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_label_components");
}

static int pair_box(const ppp_params *p, int32_t max_ps_dist, int *box, int *l1max) {
    if (max_ps_dist < 0) return fail(PPP_ERR_INVALID_ARG, "max_ps_dist < 0");
    box[0] = max_ps_dist * p->pz; box[1] = max_ps_dist * p->py; box[2] = max_ps_dist * p->px;
    *l1max = 2 * (p->pz + p->py + p->px);
    return PPP_OK;
}

int ppp_patch_pairs_count(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                          int64_t *d_counts, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n == 0) return PPP_OK;
    if (!d_sorted_zyx || !d_counts) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    int box[3], l1max;
    PPP_TRY(pair_box(p, max_ps_dist, box, &l1max));
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pairs_count(d_sorted_zyx, n, box, l1max, d_counts, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_pairs_count");
}

int ppp_patch_pairs_count_subset(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                                 const int64_t *d_subset, int64_t m, int64_t *d_counts,
                                 const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n == 0 || m == 0) return PPP_OK;
    if (!d_sorted_zyx || !d_counts || !d_subset) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    int box[3], l1max;
    PPP_TRY(pair_box(p, max_ps_dist, box, &l1max));
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pairs_count(d_sorted_zyx, n, box, l1max, d_counts, (hipStream_t)stream, d_subset, m);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_pairs_count_subset");
}

int ppp_patch_pairs_fill_subset(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                                const int64_t *d_subset, int64_t m, const int64_t *d_local_offsets,
                                const int64_t *d_global_offsets, int64_t n_local_rows,
                                int64_t n_rows_total, int32_t include_single, uint32_t *d_rows,
                                int64_t *d_row_ids, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n == 0 || m == 0) return PPP_OK;
    if (!d_sorted_zyx || !d_subset || !d_local_offsets || !d_global_offsets || !d_rows || !d_row_ids)
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    int box[3], l1max;
    PPP_TRY(pair_box(p, max_ps_dist, box, &l1max));
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pairs_subset(d_sorted_zyx, n, box, l1max, d_subset, m, d_local_offsets,
                                            d_global_offsets, n_local_rows, n_rows_total, include_single,
                                            d_rows, (long long *)d_row_ids, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_pairs_fill_subset");
}

int ppp_patch_pairs_fill(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                         const int64_t *d_offsets, int64_t n_pair_rows, int32_t include_single,
                         uint32_t *d_rows, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n == 0) return PPP_OK;
    if (!d_sorted_zyx || !d_offsets || !d_rows) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    int box[3], l1max;
    PPP_TRY(pair_box(p, max_ps_dist, box, &l1max));
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pairs_fill(d_sorted_zyx, n, box, l1max, d_offsets, n_pair_rows, include_single, d_rows, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_pairs_fill");
}

int ppp_patch_pairs_count_slices(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                                 int64_t *d_counts, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(slices_geo(p, 1, &G));
    if (n == 0) return PPP_OK;
    if (!d_sorted_zyx || !d_counts) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    int box[3], l1max;
    PPP_TRY(pair_box(p, max_ps_dist, box, &l1max));
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pairs_count(d_sorted_zyx, n, box, l1max, d_counts, (hipStream_t)stream,
                                           nullptr, 0, true);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_pairs_count_slices");
}

int ppp_patch_pairs_fill_slices(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                                const int64_t *d_offsets, int64_t n_pair_rows, int32_t include_single,
                                uint32_t *d_rows, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(slices_geo(p, 1, &G));
    if (n == 0) return PPP_OK;
    if (!d_sorted_zyx || !d_offsets || !d_rows) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    int box[3], l1max;
    PPP_TRY(pair_box(p, max_ps_dist, box, &l1max));
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pairs_fill(d_sorted_zyx, n, box, l1max, d_offsets, n_pair_rows, include_single,
                                          d_rows, (hipStream_t)stream, true);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_pairs_fill_slices");
}

int ppp_label_slice_renumber(const uint32_t *d_nodes, uint64_t n_nodes, int32_t *d_labels,
                             int32_t *d_slice_min, int32_t *d_slice_max, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(slices_geo(p, 1, &G));
    if ((n_nodes && (!d_nodes || !d_labels)) || !d_slice_min || !d_slice_max)
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_label_slice_renumber(d_nodes, n_nodes, d_labels, d_slice_min, d_slice_max, G,
                                                    (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_label_slice_renumber");
}

int ppp_pair_sort_keys(const uint32_t *d_rows, uint64_t n_rows, int64_t *d_keys,
                       const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n_rows == 0) return PPP_OK;
    if (!d_rows || !d_keys) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pair_keys(d_rows, n_rows, d_keys, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_pair_sort_keys");
}

int ppp_pair_group_keys(const uint32_t *d_rows, uint64_t n_rows, int64_t *d_keys,
                        const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n_rows == 0) return PPP_OK;
    if (!d_rows || !d_keys) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if ((int64_t)(4 * G.pz + 1) * (4 * G.py + 1) * (4 * G.px + 1) > (1 << 17))
        return fail(PPP_ERR_UNSUPPORTED, "patch shape too large for ppp_pair_group_keys");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pair_group_keys(d_rows, n_rows, d_keys, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_pair_group_keys");
}

int ppp_paint_instances(const void *d_pred, int pred_dtype, const uint32_t *d_nodes,
                        const uint32_t *d_labels, uint64_t n_nodes, uint32_t *d_instances,
                        const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (n_nodes == 0) return PPP_OK;
    if (!d_pred || !d_nodes || !d_labels || !d_instances) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_paint(d_pred, pred_dtype, d_nodes, d_labels, n_nodes, d_instances, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_paint_instances");
}

// ---- no_overlap_per_channel (ppp_pack_channels.hip) ----------------------------------------------
static int pack_own_box(const ppp_box *own, const ppp::Geo &G, ppp_box *b) {
    if (own) *b = *own;
    else { b->z0 = b->y0 = b->x0 = 0; b->z1 = G.Z; b->y1 = G.Y; b->x1 = G.X; }
    if (b->z0 < 0 || b->y0 < 0 || b->x0 < 0 || b->z1 > G.Z || b->y1 > G.Y || b->x1 > G.X ||
        b->z1 < b->z0 || b->y1 < b->y0 || b->x1 < b->x0)
        return fail(PPP_ERR_INVALID_ARG, "own box outside the frame");
    return PPP_OK;
}

int64_t ppp_pack_scan_workspace_bytes(const ppp_params *p, const ppp_box *own) {
    ppp::Geo G;
    ppp_box b;
    int rc = make_geo(p, &G);
    if (rc == PPP_OK) rc = pack_own_box(own, G, &b);
    return rc != PPP_OK ? rc : (int64_t)ppp::pack_scan_workspace_bytes(G, b);
}

int ppp_pack_scan_count(const void *d_pred, int pred_dtype, const uint32_t *d_nodes, const uint32_t *d_labels,
                        uint64_t n_nodes, uint32_t n_labels, const ppp_box *own, uint64_t *d_sizes,
                        int64_t *n_pairs, void *d_work, const ppp_params *p, void *stream) {
    ppp::Geo G;
    ppp_box b;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    PPP_TRY(pack_own_box(own, G, &b));
    if (!n_pairs || !d_work || !d_sizes || (n_nodes > 0 && (!d_pred || !d_nodes || !d_labels)))
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    long long np = 0;
    hipError_t e = ppp::run_pack_scan_count(d_pred, pred_dtype, d_nodes, d_labels, n_nodes, n_labels, b,
                                            (unsigned long long *)d_sizes, &np, d_work, G, (hipStream_t)stream);
    *n_pairs = np;
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_pack_scan_count");
}

int ppp_pack_scan_fill(const void *d_pred, int pred_dtype, const ppp_box *own, uint64_t *d_pairs, int64_t n_pairs,
                       void *d_work, const ppp_params *p, void *stream) {
    ppp::Geo G;
    ppp_box b;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    PPP_TRY(pack_own_box(own, G, &b));
    if (n_pairs < 0) return fail(PPP_ERR_INVALID_ARG, "n_pairs must be >= 0");
    if (n_pairs == 0) return PPP_OK;
    if (!d_pred || !d_pairs || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_pack_scan_fill(d_pred, pred_dtype, b, (unsigned long long *)d_pairs, n_pairs, d_work, G,
                                           (hipStream_t)stream);
    if (e == hipErrorInvalidValue)
        return fail(PPP_ERR_INVALID_ARG, "ppp_pack_scan_fill: n_pairs / workspace are not those of ppp_pack_scan_count");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_pack_scan_fill");
}

int ppp_paint_instances_channels(const void *d_pred, int pred_dtype, const uint32_t *d_nodes,
                                 const uint32_t *d_labels, uint64_t n_nodes, const uint32_t *d_chan,
                                 uint32_t n_labels, uint32_t n_channels, uint32_t *d_out,
                                 const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (n_nodes == 0 || n_channels == 0) return PPP_OK;
    if (!d_pred || !d_nodes || !d_labels || !d_chan || !d_out) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_paint_channels(d_pred, pred_dtype, d_nodes, d_labels, n_nodes, d_chan, n_labels, n_channels,
                                              d_out, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_paint_instances_channels");
}

// ---- the reference's NumPy-semantics stages (cuda=False) -----------------------------------------
int64_t ppp_np_vote_planes(const ppp_params *p) {
    ppp::Geo G;
    if (!p || make_geo(p, &G) != PPP_OK) return -1;
    return (int64_t)G.n_planes + 1;
}

int ppp_np_consensus(const void *d_pred, int pred_dtype, const uint8_t *d_foreground, int16_t *d_votes,
                     const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || !d_foreground || !d_votes) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_np_consensus(d_pred, pred_dtype, d_foreground, d_votes, G, p->th, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_np_consensus");
}

int ppp_np_rank_patches(const void *d_pred, int pred_dtype, const uint8_t *d_foreground, const int16_t *d_votes,
                        int32_t *d_score, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || !d_foreground || !d_votes || !d_score) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.C > 32768) return fail(PPP_ERR_UNSUPPORTED, "patch too large for ppp_np_rank_patches");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_np_rank(d_pred, pred_dtype, d_foreground, d_votes, d_score, G, p->th, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_np_rank_patches");
}

int ppp_np_patch_graph(const void *d_pred, int pred_dtype, const uint8_t *d_mask, const int16_t *d_votes,
                       const int32_t *d_rows, uint64_t n_rows, int64_t *d_weight, int32_t *d_count,
                       const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (n_rows == 0) return PPP_OK;
    if (!d_pred || !d_mask || !d_votes || !d_rows || !d_weight || !d_count) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.C > 16384) return fail(PPP_ERR_UNSUPPORTED, "patch too large for ppp_np_patch_graph");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_np_graph(d_pred, pred_dtype, d_mask, d_votes, d_rows, n_rows, (long long *)d_weight, d_count,
                                        G, p->th, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_np_patch_graph");
}

int ppp_paint_patch_rows(const void *d_rows, int rows_dtype, const uint32_t *d_nodes,
                         const uint32_t *d_labels, uint64_t n_nodes, uint32_t *d_instances,
                         const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(rows_dtype));
    if (n_nodes == 0) return PPP_OK;
    if (!d_rows || !d_nodes || !d_labels || !d_instances) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_paint_rows(d_rows, rows_dtype, d_nodes, d_labels, n_nodes, d_instances, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_paint_patch_rows");
}

int ppp_cons_to_reference(const float *d_cons_compact, float *d_cons_reference,
                          const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (!d_cons_compact || !d_cons_reference) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.BV != G.V) return fail(PPP_ERR_INVALID_ARG, "whole-volume consensus required");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_cons_to_reference(d_cons_compact, d_cons_reference, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_cons_to_reference");
}

int ppp_cons_to_voxel_major(const float *d_cons_compact, float *d_cons_voxel_major,
                            const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (!d_cons_compact || !d_cons_voxel_major) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.layout == PPP_CONS_REFERENCE) return fail(PPP_ERR_INVALID_ARG, "source must be a COMPACT consensus");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_cons_to_voxel_major(d_cons_compact, d_cons_voxel_major, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_cons_to_voxel_major");
}

int ppp_cons_planes_to_rows(const float *d_planes, const ppp_box *planes_box, float *d_rows, const ppp_params *p,
                            void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (!d_planes || !d_rows || !planes_box) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.layout != PPP_CONS_VOXEL_MAJOR || G.ring) return fail(PPP_ERR_INVALID_ARG, "params must describe VOXEL_MAJOR rows of a plain box");
    const ppp_box &b = p->cons_box, &q = *planes_box;
    if (q.z1 <= q.z0 || q.y1 <= q.y0 || q.x1 <= q.x0 || b.z0 < q.z0 || b.y0 < q.y0 || b.x0 < q.x0 || b.z1 > q.z1 ||
        b.y1 > q.y1 || b.x1 > q.x1)
        return fail(PPP_ERR_INVALID_ARG, "the planes' box must hold cons_box (the rows' box)");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_cons_planes_to_rows(d_planes, q, d_rows, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_cons_planes_to_rows");
}

int ppp_patch_bits(const void *d_pred, int pred_dtype, const uint32_t *d_centres, uint64_t n,
                   double thresh, uint32_t *d_bits, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (n == 0) return PPP_OK;
    if (!d_pred || !d_centres || !d_bits) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_patch_bits(d_pred, pred_dtype, d_centres, n, (float)thresh, d_bits, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_bits");
}

int ppp_patch_bits_volume(const void *d_pred, int pred_dtype, double thresh, uint32_t *d_bits_vol,
                          const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || !d_bits_vol) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_patch_bits_volume(d_pred, pred_dtype, (float)thresh, d_bits_vol, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_bits_volume");
}

int ppp_synth_pred(const int32_t *d_labels, void *d_pred, int pred_dtype, uint32_t seed,
                   float hi, float lo, float noise, uint64_t voxel_offset, const ppp_params *p,
                   void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype_f32_f16(pred_dtype, "ppp_synth_pred"));
    if (!d_labels || !d_pred) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_synth(d_labels, d_pred, pred_dtype, seed, hi, lo, noise, voxel_offset, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_synth_pred");
}

int ppp_synth_pred_box(const int32_t *d_labels, const int32_t *label_box, void *d_pred, int pred_dtype,
                       uint32_t seed, float hi, float lo, float noise, const int32_t *global_dims,
                       const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype_f32_f16(pred_dtype, "ppp_synth_pred_box"));
    if (!d_labels || !d_pred || !label_box || !global_dims) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    const int lo3[3] = {G.oz, G.oy, G.ox}, ext[3] = {G.Z, G.Y, G.X}, rad[3] = {G.rz, G.ry, G.rx};
    for (int a = 0; a < 3; ++a) {
        const int need_lo = lo3[a] - rad[a] < 0 ? 0 : lo3[a] - rad[a];
        const int need_hi = lo3[a] + ext[a] + rad[a] > global_dims[a] ? global_dims[a] : lo3[a] + ext[a] + rad[a];
        if (lo3[a] < 0 || lo3[a] + ext[a] > global_dims[a] || label_box[a] > need_lo || label_box[3 + a] < need_hi)
            return fail(PPP_ERR_INVALID_ARG, "label box must hold the prediction box grown by the patch radius");
    }
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_synth_box(d_labels, label_box, d_pred, pred_dtype, seed, hi, lo, noise, global_dims,
                                         G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_synth_pred_box");
}

int ppp_counter_calibration(const void *d_src, int src_dtype, int64_t n_read, float *d_dst, int64_t n_write,
                            void *stream) {
    PPP_TRY(check_dtype_f32_f16(src_dtype, "ppp_counter_calibration"));
    if ((n_read > 0 && !d_src) || !d_dst || n_read < 0 || n_write < 0) return fail(PPP_ERR_INVALID_ARG, "bad argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_counter_calibration(d_src, src_dtype, n_read, d_dst, n_write, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_counter_calibration");
}

int ppp_pred_check(const void *d_pred, int pred_dtype, int64_t n_values, int32_t *d_unclean, const ppp_params *p,
                   void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_unclean || n_values < 0 || (n_values > 0 && !d_pred)) return fail(PPP_ERR_INVALID_ARG, "bad argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pred_check(d_pred, pred_dtype, n_values, G, d_unclean, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_pred_check");
}

/* ---- the fused pre-pass over the prediction (ppp_prepass.hip) ---- */
// (before S1 there is no consensus box yet: the pre-pass asks for none, the prepared ranking call checks its own)
static int prepass_box(const ppp_box *score_box, const ppp_params *p, ppp_box *sb) {
    *sb = ppp_box{0, 0, 0, p->Z, p->Y, p->X};
    if (score_box) *sb = *score_box;
    if (sb->z0 < 0 || sb->y0 < 0 || sb->x0 < 0 || sb->z1 > p->Z || sb->y1 > p->Y || sb->x1 > p->X ||
        sb->z1 <= sb->z0 || sb->y1 <= sb->y0 || sb->x1 <= sb->x0)
        return fail(PPP_ERR_INVALID_ARG, "score_box outside the volume");
    return PPP_OK;
}

int64_t ppp_pred_prepass_workspace_bytes(const ppp_box *score_box, const ppp_params *p) {
    ppp::Geo G;
    ppp_box sb;
    if (!p || make_geo(p, &G) != PPP_OK) return -1;
    if (!ppp::pred_prepass_supported(G)) return 0;
    if (prepass_box(score_box, p, &sb) != PPP_OK) return -1;
    return (int64_t)ppp::pred_prepass_workspace_bytes(sb, G);
}

int ppp_pred_prepass_layout(const ppp_box *score_box, const ppp_params *p, int64_t *offsets) {
    ppp::Geo G;
    ppp_box sb;
    PPP_TRY(make_geo(p, &G));
    if (!offsets) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (!ppp::pred_prepass_supported(G)) return fail(PPP_ERR_UNSUPPORTED, "ppp_pred_prepass: cubic patches of 5 / 7 / 9 only");
    PPP_TRY(prepass_box(score_box, p, &sb));
    char base;                                            // (any base: only the differences count)
    ppp::Carver c(&base);
    const ppp::PrepassWork W = ppp::pred_prepass_layout(c, sb, G);
    offsets[0] = (char *)W.M - &base; offsets[1] = (char *)W.info - &base; offsets[2] = (char *)W.valid - &base;
    offsets[3] = (char *)W.bits_vol - &base; offsets[4] = (char *)W.unclean - &base;
    return PPP_OK;
}

int ppp_pred_prepass(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, double fc_threshold, float *d_score,
                     const ppp_box *score_box, void *d_work, const ppp_params *p, void *stream) {
    ppp::Geo G;
    ppp_box sb;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype(pred_dtype));
    if (!d_pred || !d_score || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (G.use_overlap && !d_overlap) return fail(PPP_ERR_INVALID_ARG, "use_overlap set but d_overlap is NULL");
    if (((uintptr_t)d_work & 15) != 0) return fail(PPP_ERR_INVALID_ARG, "ppp_pred_prepass: d_work must be 16-byte aligned");
    if (!ppp::pred_prepass_supported(G))
        return fail(PPP_ERR_UNSUPPORTED, "ppp_pred_prepass: cubic patches of 5 / 7 / 9, no count_pos_neg, no ring "
                                         "(use ppp_pred_check, ppp_rank_patches_vm and ppp_patch_bits_volume otherwise)");
    PPP_TRY(prepass_box(score_box, p, &sb));
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_pred_prepass(d_pred, pred_dtype, d_overlap, (float)fc_threshold, d_score, sb, d_work, G,
                                            (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(PPP_ERR_UNSUPPORTED, "ppp_pred_prepass: a grid the device would not run whole");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_pred_prepass");
}

int64_t ppp_rank_prepared_workspace_bytes(const ppp_params *p) {
    ppp::Geo G;
    if (!p || make_geo(p, &G) != PPP_OK) return -1;
    if (!ppp::rank_wg_supported(G) || G.ring) return 0;
    return (int64_t)ppp::rank_wg_prepared_workspace_bytes(G);
}

int ppp_rank_patches_vm_prepared(const float *d_cons_vm, float *d_score, const ppp_box *score_box, void *d_prepass_work,
                                 void *d_work, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (!d_cons_vm || !d_score || !d_prepass_work || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (!ppp::rank_wg_supported(G) || G.ring)
        return fail(PPP_ERR_UNSUPPORTED, "ppp_rank_patches_vm_prepared: VOXEL_MAJOR rows of a plain box, cubic patches of 5 / 7 / 9");
    ppp_box sb;
    PPP_TRY(rank_box(score_box, p, G, &sb));
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_rank_wg_prepared(d_cons_vm, d_score, sb, d_prepass_work, d_work, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_rank_patches_vm_prepared");
}

int ppp_patch_bits_from_table(const uint32_t *d_bits_vol, const uint32_t *d_centres, uint64_t n, uint32_t *d_bits,
                              const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (n == 0) return PPP_OK;
    if (!d_bits_vol || !d_centres || !d_bits) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_patch_bits_from_table(d_bits_vol, d_centres, n, d_bits, G, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(PPP_ERR_UNSUPPORTED, "ppp_patch_bits_from_table: more rows than one launch copies");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_bits_from_table");
}

int ppp_decode_tail(const float *d_x, int64_t n, int32_t fmaps, int32_t side, const float *d_w1, float b1,
                    const float *d_w2, float b2, const float *d_w3, float b3, const int64_t *d_dst,
                    void *d_pred, int pred_dtype, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    PPP_TRY(check_dtype_f32_f16(pred_dtype, "ppp_decode_tail"));
    if (n <= 0) return PPP_OK;
    if (!d_x || !d_w1 || !d_w2 || !d_w3 || !d_dst || !d_pred) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_decode_tail(d_x, n, fmaps, side, d_w1, b1, d_w2, b2, d_w3, b3,
                                           (const long long *)d_dst, d_pred, pred_dtype, G, (hipStream_t)stream);
    if (e == hipErrorNotSupported)
        return fail(PPP_ERR_UNSUPPORTED, "ppp_decode_tail serves the shipped decoder tail only: 64 feature maps "
                                         "at 4^3, 3^3 kernels, 7^3 patches");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_decode_tail");
}

int ppp_decode_tail_rows(const float *d_x, int64_t n, int32_t fmaps, int32_t side, const float *d_w1, float b1,
                         const float *d_w2, float b2, const float *d_w3, float b3, const int64_t *d_dst,
                         void *d_rows, int rows_dtype, int32_t C, void *stream) {
    PPP_TRY(check_dtype_f32_f16(rows_dtype, "ppp_decode_tail_rows"));
    if (n <= 0) return PPP_OK;
    if (!d_x || !d_w1 || !d_w2 || !d_w3 || !d_dst || !d_rows) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = C != 343 ? hipErrorNotSupported
                            : ppp::launch_decode_tail_rows(d_x, n, fmaps, side, d_w1, b1, d_w2, b2, d_w3, b3,
                                                           (const long long *)d_dst, d_rows, rows_dtype, (hipStream_t)stream);
    if (e == hipErrorNotSupported)
        return fail(PPP_ERR_UNSUPPORTED, "ppp_decode_tail_rows serves the shipped decoder tail only: 64 feature maps "
                                         "at 4^3, 3^3 kernels, rows of 7^3 = 343 values");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_decode_tail_rows");
}

/* ---- a prediction kept as rows of the mask voxels (ppp_rows.hip) ---- */
static int rows_volume(int32_t Z, int32_t Y, int32_t X, long long *V) {
    if (Z <= 0 || Y <= 0 || X <= 0) return fail(PPP_ERR_INVALID_ARG, "bad volume %d x %d x %d", Z, Y, X);
    *V = (long long)Z * Y * X;
    if (*V >= (1ll << 31)) return fail(PPP_ERR_UNSUPPORTED, "volumes of 2^31 voxels or more are not supported");
    return PPP_OK;
}

int64_t ppp_rows_index_bytes(int32_t Z, int32_t Y, int32_t X) {
    long long V;
    int rc = rows_volume(Z, Y, X, &V);
    return rc != PPP_OK ? rc : (int64_t)ppp::rows_index_bytes(V);
}

int ppp_rows_index_build(const uint8_t *d_mask, int32_t Z, int32_t Y, int32_t X, void *d_index, int64_t *n_rows,
                         void *stream) {
    long long V;
    PPP_TRY(rows_volume(Z, Y, X, &V));
    if (!d_mask || !d_index || !n_rows) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if ((uintptr_t)d_index & 7) return fail(PPP_ERR_INVALID_ARG, "ppp_rows_index_build: the index must be 8-byte aligned");
    PPP_TRY(need_device());
    long long n = 0;
    hipError_t e = ppp::run_rows_index_build(d_mask, V, d_index, &n, (hipStream_t)stream);
    *n_rows = n;
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_rows_index_build");
}

static int rows_move(bool expand, const char *who, void *d_rows, int dtype, int32_t C, const void *d_index, int32_t Z,
                     int32_t Y, int32_t X, const ppp_box *box, void *d_pred_box, void *stream) {
    long long V;
    PPP_TRY(rows_volume(Z, Y, X, &V));
    PPP_TRY(check_dtype(dtype));
    if (C <= 0) return fail(PPP_ERR_INVALID_ARG, "%s: rows of %d values", who, C);
    if (!d_index || !box || !d_pred_box) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (box->z0 < 0 || box->y0 < 0 || box->x0 < 0 || box->z1 > Z || box->y1 > Y || box->x1 > X || box->z1 <= box->z0 ||
        box->y1 <= box->y0 || box->x1 <= box->x0)
        return fail(PPP_ERR_INVALID_ARG, "%s: box outside the volume or empty", who);
    // (the 2-byte forms move aligned dwords where they can: both buffers must start on one)
    if (((uintptr_t)d_rows & 3) || ((uintptr_t)d_pred_box & 3) || ((uintptr_t)d_index & 7))
        return fail(PPP_ERR_INVALID_ARG, "%s: rows and box must be 4-byte aligned, the index 8-byte aligned", who);
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_rows_move(expand, d_rows, dtype == PPP_F32 ? 4 : 2, C, d_index, Z, Y, X, *box, d_pred_box,
                                         (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, who);
}

int ppp_rows_expand(const void *d_rows, int dtype, int32_t C, const void *d_index, int32_t Z, int32_t Y, int32_t X,
                    const ppp_box *box, void *d_pred_box, void *stream) {
    return rows_move(true, "ppp_rows_expand", const_cast<void *>(d_rows), dtype, C, d_index, Z, Y, X, box, d_pred_box, stream);
}

int ppp_rows_compact(const void *d_pred_box, int dtype, int32_t C, const ppp_box *box, const void *d_index, int32_t Z,
                     int32_t Y, int32_t X, void *d_rows, void *stream) {
    return rows_move(false, "ppp_rows_compact", d_rows, dtype, C, d_index, Z, Y, X, box, const_cast<void *>(d_pred_box),
                     stream);
}

int64_t ppp_cover_workspace_bytes(int64_t n, const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    return (int64_t)ppp::cover_workspace_bytes(n < 0 ? 0 : n, G);
}

static int cover_pass_impl(uint8_t *d_mask, const uint32_t *d_bits, int64_t first_voxel, const int64_t *d_lin,
                           int64_t n, int32_t pix_th, int32_t *d_state, int32_t *d_cleared, void *d_work,
                           const ppp_params *p, void *stream, int32_t *rounds, const char *who,
                           uint32_t *d_mark_bits = nullptr, bool marked = false) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (rounds) *rounds = 0;
    if (marked && !d_mark_bits) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (marked && (G.Y < 7 || G.X < 7))
        return fail(PPP_ERR_UNSUPPORTED, "%s needs y and x axes of at least 7 voxels (the mark box wraps on shorter ones)", who);
    if (n <= 0) return PPP_OK;
    if (n > 0x7F000000LL) return fail(PPP_ERR_INVALID_ARG, "too many ranked patches for one cover pass");
    if (G.px > 32) return fail(PPP_ERR_UNSUPPORTED, "%s needs patch rows of at most 32 voxels", who);
    if (!d_mask || !d_bits || !d_lin || !d_state || !d_cleared || !d_work)
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    int r = 0;
    hipError_t e = ppp::run_cover_pass(d_mask, d_bits, first_voxel, (const long long *)d_lin, n, pix_th, d_state,
                                       d_cleared, d_work, G, (hipStream_t)stream, &r, d_mark_bits);
    if (rounds) *rounds = r;
    return e == hipSuccess ? PPP_OK : hip_fail(e, who);
}

int ppp_cover_pass(uint8_t *d_mask, const uint32_t *d_bits, const int64_t *d_lin, int64_t n,
                   int32_t pix_th, int32_t *d_state, int32_t *d_cleared, void *d_work,
                   const ppp_params *p, void *stream, int32_t *rounds) {
    return cover_pass_impl(d_mask, d_bits, -1, d_lin, n, pix_th, d_state, d_cleared, d_work, p, stream, rounds,
                           "ppp_cover_pass");
}

int ppp_cover_pass_voxel_bits(uint8_t *d_mask, const uint32_t *d_bits_by_voxel, int64_t first_voxel,
                              const int64_t *d_lin, int64_t n, int32_t pix_th, int32_t *d_state,
                              int32_t *d_cleared, void *d_work, const ppp_params *p, void *stream,
                              int32_t *rounds) {
    if (first_voxel < 0) return fail(PPP_ERR_INVALID_ARG, "first_voxel must be >= 0");
    return cover_pass_impl(d_mask, d_bits_by_voxel, first_voxel, d_lin, n, pix_th, d_state, d_cleared, d_work, p,
                           stream, rounds, "ppp_cover_pass_voxel_bits");
}

int ppp_cover_pass_marked(uint8_t *d_mask, const uint32_t *d_bits, const int64_t *d_lin, int64_t n,
                          int32_t pix_th, int32_t *d_state, int32_t *d_cleared, uint32_t *d_mark_bits,
                          void *d_work, const ppp_params *p, void *stream, int32_t *rounds) {
    return cover_pass_impl(d_mask, d_bits, -1, d_lin, n, pix_th, d_state, d_cleared, d_work, p, stream, rounds,
                           "ppp_cover_pass_marked", d_mark_bits, true);
}

int ppp_cover_pass_marked_voxel_bits(uint8_t *d_mask, const uint32_t *d_bits_by_voxel, int64_t first_voxel,
                                     const int64_t *d_lin, int64_t n, int32_t pix_th, int32_t *d_state,
                                     int32_t *d_cleared, uint32_t *d_mark_bits, void *d_work,
                                     const ppp_params *p, void *stream, int32_t *rounds) {
    if (first_voxel < 0) return fail(PPP_ERR_INVALID_ARG, "first_voxel must be >= 0");
    return cover_pass_impl(d_mask, d_bits_by_voxel, first_voxel, d_lin, n, pix_th, d_state, d_cleared, d_work, p,
                           stream, rounds, "ppp_cover_pass_marked_voxel_bits", d_mark_bits, true);
}

int64_t ppp_cover_mark_bits_bytes(const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    return (int64_t)ppp::cover_mark_bits_bytes(G);
}

int ppp_cover_marks_from_selected(const int64_t *d_lin, const uint8_t *d_selected, int64_t n,
                                  uint32_t *d_mark_bits, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (G.Y < 7 || G.X < 7)
        return fail(PPP_ERR_UNSUPPORTED, "ppp_cover_marks_from_selected needs y and x axes of at least 7 voxels");
    if (!d_mark_bits || (n > 0 && !d_lin)) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_cover_marks_from_selected((const long long *)d_lin, d_selected, n < 0 ? 0 : n,
                                                      d_mark_bits, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_cover_marks_from_selected");
}

int64_t ppp_mask_dilate_workspace_bytes(const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    return (int64_t)ppp::mask_dilate_workspace_bytes(G);
}

int ppp_mask_dilate(const uint8_t *d_in, uint8_t *d_out, int32_t iterations, int32_t use_z, void *d_work,
                    const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (iterations < 0) return fail(PPP_ERR_INVALID_ARG, "ppp_mask_dilate: iterations must be >= 0");
    if (!d_in || !d_out || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_mask_dilate(d_in, d_out, iterations, use_z ? 1 : 0, d_work, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_mask_dilate");
}

int ppp_minfilter_xy(const void *d_in, void *d_out, void *d_scratch, int32_t elem_bytes, const ppp_params *p,
                     void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (elem_bytes != 4 && elem_bytes != 8) return fail(PPP_ERR_INVALID_ARG, "ppp_minfilter_xy: elements of 4 or 8 bytes");
    if (!d_in || !d_out || !d_scratch || d_in == d_out) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument or d_in == d_out");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_minfilter_xy(d_in, d_scratch, d_out, elem_bytes, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_minfilter_xy");
}

int64_t ppp_rank_order_workspace_bytes(const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    return (int64_t)ppp::rank_order_workspace_bytes(G);
}

int ppp_rank_order(const float *d_score, const uint8_t *d_foreground, int64_t *d_lin,
                   float *d_rank_score, int64_t *count, void *d_work, const ppp_params *p,
                   void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (!d_score || !d_foreground || !d_lin || !count || !d_work)
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    long long n = 0;
    hipError_t e = ppp::run_rank_order(d_score, d_foreground, (long long *)d_lin, d_rank_score, &n, d_work,
                                       G, (hipStream_t)stream);
    *count = n;
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_rank_order");
}

int64_t ppp_mws_edges_workspace_bytes(int64_t n_rows, int64_t n_nodes, const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    return (int64_t)ppp::mws_edges_workspace_bytes(n_rows, n_nodes, G);
}

int ppp_mws_edges(const uint32_t *d_pairs, const float *d_aff, int64_t n_rows, const uint32_t *d_nodes,
                  int64_t n_nodes, int32_t *d_eu, int32_t *d_ev, int64_t *n_edges, void *d_work,
                  const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(make_geo(p, &G));
    if (!n_edges) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    *n_edges = 0;
    if (n_rows <= 0) return PPP_OK;
    if (!d_pairs || !d_aff || !d_nodes || !d_eu || !d_ev || !d_work)
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    long long ne = 0;
    hipError_t e = ppp::run_mws_edges(d_pairs, d_aff, n_rows, d_nodes, n_nodes, d_eu, d_ev, &ne, d_work, G,
                                      (hipStream_t)stream);
    *n_edges = ne;
    if (e == hipErrorInvalidValue)
        return fail(PPP_ERR_INVALID_ARG, "ppp_mws_edges: too many rows, or a row names a voxel that is not a node");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_mws_edges");
}

int64_t ppp_thin_workspace_bytes(int64_t n, const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    return (int64_t)ppp::thin_workspace_bytes(n < 0 ? 0 : n, G);
}

static int thin_cover_impl(const uint8_t *d_mask, const uint32_t *d_bits, const int64_t *d_lin, int64_t n,
                           uint8_t *d_keep, void *d_work, const ppp_params *p, void *stream,
                           int32_t *rounds, const int64_t *h_slice_interior) {
    ppp::Geo G;
    PPP_TRY(slices_geo(p, h_slice_interior != nullptr, &G));
    if (rounds) *rounds = 0;
    if (n <= 0) return PPP_OK;
    if (n > 0x7F000000LL) return fail(PPP_ERR_INVALID_ARG, "too many selected patches for ppp_thin_cover");
    if (G.px > 32) return fail(PPP_ERR_UNSUPPORTED, "ppp_thin_cover needs patch rows of at most 32 voxels");
    if (!d_mask || !d_bits || !d_lin || !d_keep || !d_work)
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    int r = 0;
    hipError_t e = ppp::run_thin_cover(d_mask, d_bits, (const long long *)d_lin, n, d_keep, d_work, G,
                                       (hipStream_t)stream, &r, (const long long *)h_slice_interior);
    if (rounds) *rounds = r;
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_thin_cover");
}

int ppp_thin_cover(const uint8_t *d_mask, const uint32_t *d_bits, const int64_t *d_lin, int64_t n,
                   uint8_t *d_keep, void *d_work, const ppp_params *p, void *stream,
                   int32_t *rounds) {
    return thin_cover_impl(d_mask, d_bits, d_lin, n, d_keep, d_work, p, stream, rounds, nullptr);
}

int ppp_thin_cover_slices(const uint8_t *d_mask, const uint32_t *d_bits, const int64_t *d_lin, int64_t n,
                          uint8_t *d_keep, void *d_work, const int64_t *h_slice_interior,
                          const ppp_params *p, void *stream, int32_t *rounds) {
    if (!h_slice_interior) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    return thin_cover_impl(d_mask, d_bits, d_lin, n, d_keep, d_work, p, stream, rounds, h_slice_interior);
}

/* ---- sharded cover: the rounds of ppp_cover_pass one step at a time on a rank's z-range ---- */
static int cover_geo(const ppp_params *p, ppp::Geo *G) {
    PPP_TRY(make_geo(p, G));
    if (G->px > 32) return fail(PPP_ERR_UNSUPPORTED, "the cover needs patch rows of at most 32 voxels");
    return need_device();
}

int ppp_cover_open(const uint8_t *d_mask, const int64_t *d_lin, const int32_t *d_rank_id, int64_t n,
                   const int32_t *d_state, int32_t *d_cleared, void *d_work, const ppp_params *p,
                   void *stream) {
    ppp::Geo G;
    PPP_TRY(cover_geo(p, &G));
    if (!d_mask || !d_work || (n > 0 && (!d_lin || !d_rank_id || !d_state || !d_cleared)))
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    hipError_t e = ppp::cover_open(d_mask, (const long long *)d_lin, d_rank_id, n, d_state, d_cleared,
                                   d_work, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_cover_open");
}

int ppp_cover_step(int32_t what, const uint32_t *d_bits, int32_t pix_th, int32_t *d_state,
                   int32_t *d_cleared, void *d_work, int32_t global_z, const ppp_params *p,
                   void *stream) {
    ppp::Geo G;
    PPP_TRY(cover_geo(p, &G));
    if (!d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    hipError_t e;
    if (what == PPP_COVER_COUNT) e = ppp::cover_step_count(d_bits, pix_th, d_state, d_work, G, (hipStream_t)stream);
    else if (what == PPP_COVER_FILTER) e = ppp::round_step_filter<int32_t>(d_work, G, (hipStream_t)stream);
    else if (what == PPP_COVER_SELECT) e = ppp::cover_step_select(d_bits, pix_th, d_state, d_cleared, d_work, global_z, G, (hipStream_t)stream);
    else return fail(PPP_ERR_INVALID_ARG, "unknown cover step %d", what);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_cover_step");
}

/* alive, close and zone are the same steps for the cover (32-bit ranks) and the thinning (64-bit keys) */
static int round_alive(bool thin, void *d_work, const ppp_params *p, void *stream, int32_t *alive) {
    ppp::Geo G;
    PPP_TRY(cover_geo(p, &G));
    if (!d_work || !alive) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    hipError_t e = thin ? ppp::round_alive<long long>(d_work, G, alive, (hipStream_t)stream)
                        : ppp::round_alive<int32_t>(d_work, G, alive, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, thin ? "ppp_thin_alive" : "ppp_cover_alive");
}

static int round_close(bool thin, uint8_t *d_mask, void *d_work, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(cover_geo(p, &G));
    if (!d_mask || !d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    hipError_t e = thin ? ppp::round_close<long long>(d_mask, d_work, G, (hipStream_t)stream)
                        : ppp::round_close<int32_t>(d_mask, d_work, G, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, thin ? "ppp_thin_close" : "ppp_cover_close");
}

static int round_zone(bool thin, int32_t import, void *d_work, int32_t z_lo, int32_t z_hi, int32_t own_lo, int32_t own_hi,
                      void *d_key, uint8_t *d_mask, uint8_t *d_clean, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(cover_geo(p, &G));
    if (!d_work || z_lo < 0 || z_hi > G.Z || z_lo > z_hi || ((d_mask == nullptr) != (d_clean == nullptr)))
        return fail(PPP_ERR_INVALID_ARG, "bad zone");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = thin ? ppp::round_zone(import != 0, d_work, z_lo, z_hi, own_lo, own_hi, (long long *)d_key, d_mask, d_clean, G, s)
                        : ppp::round_zone(import != 0, d_work, z_lo, z_hi, own_lo, own_hi, (int32_t *)d_key, d_mask, d_clean, G, s);
    return e == hipSuccess ? PPP_OK : hip_fail(e, thin ? "ppp_thin_zone" : "ppp_cover_zone");
}

int ppp_cover_alive(void *d_work, const ppp_params *p, void *stream, int32_t *alive) {
    return round_alive(false, d_work, p, stream, alive);
}

int ppp_cover_close(uint8_t *d_mask, void *d_work, const ppp_params *p, void *stream) {
    return round_close(false, d_mask, d_work, p, stream);
}

int ppp_cover_zone(int32_t import, void *d_work, int32_t z_lo, int32_t z_hi, int32_t own_lo,
                   int32_t own_hi, int32_t *d_rank, uint8_t *d_mask, uint8_t *d_clean,
                   const ppp_params *p, void *stream) {
    return round_zone(false, import, d_work, z_lo, z_hi, own_lo, own_hi, d_rank, d_mask, d_clean, p, stream);
}

/* ---- sharded thinning: the rounds of ppp_thin_cover one step at a time on a rank's z-range ---- */
int64_t ppp_thin_shard_workspace_bytes(const ppp_params *p) {
    ppp::Geo G;
    if (make_geo(p, &G) != PPP_OK) return -1;
    return (int64_t)ppp::thin_shard_workspace_bytes(G);
}

int ppp_thin_open(const uint8_t *d_mask, const int64_t *d_lin, const int32_t *d_index, int64_t n, int32_t *d_state,
                  int32_t *d_count, int32_t *d_cleared, void *d_work, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(cover_geo(p, &G));
    if (!d_mask || !d_work || (n > 0 && (!d_lin || !d_index || !d_state || !d_count || !d_cleared)))
        return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    hipError_t e = ppp::thin_open(d_mask, (const long long *)d_lin, d_index, n, d_state, d_count, d_cleared, d_work, G,
                                  (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_thin_open");
}

int ppp_thin_step(int32_t what, const uint32_t *d_bits, int32_t *d_state, int32_t *d_count, int32_t *d_cleared,
                  void *d_work, int32_t global_z, const ppp_params *p, void *stream) {
    ppp::Geo G;
    PPP_TRY(cover_geo(p, &G));
    if (!d_work) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    hipError_t e;
    if (what == PPP_COVER_COUNT) e = ppp::thin_step_count(d_bits, d_state, d_work, G, (hipStream_t)stream);
    else if (what == PPP_COVER_FILTER) e = ppp::round_step_filter<long long>(d_work, G, (hipStream_t)stream);
    else if (what == PPP_COVER_SELECT) e = ppp::thin_step_select(d_bits, d_state, d_count, d_cleared, d_work, global_z, G, (hipStream_t)stream);
    else return fail(PPP_ERR_INVALID_ARG, "unknown thinning step %d", what);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_thin_step");
}

int ppp_thin_alive(void *d_work, const ppp_params *p, void *stream, int32_t *alive) {
    return round_alive(true, d_work, p, stream, alive);
}

int ppp_thin_close(uint8_t *d_mask, void *d_work, const ppp_params *p, void *stream) {
    return round_close(true, d_mask, d_work, p, stream);
}

int ppp_thin_zone(int32_t import, void *d_work, int32_t z_lo, int32_t z_hi, int32_t own_lo, int32_t own_hi,
                  int64_t *d_key, uint8_t *d_mask, uint8_t *d_clean, const ppp_params *p, void *stream) {
    return round_zone(true, import, d_work, z_lo, z_hi, own_lo, own_hi, d_key, d_mask, d_clean, p, stream);
}

/* ---- post-steps of the label driver (ppp_postprocess.hip) ---- */
static int post_volume(int32_t Z, int32_t Y, int32_t X, long long *V) {
    if (Z <= 0 || Y <= 0 || X <= 0) return fail(PPP_ERR_INVALID_ARG, "bad volume %d x %d x %d", Z, Y, X);
    *V = (long long)Z * Y * X;
    if (*V >= (1ll << 31)) return fail(PPP_ERR_UNSUPPORTED, "volumes of 2^31 voxels or more are not supported");
    return PPP_OK;
}

int64_t ppp_post_compact_ids_workspace_bytes(int64_t n, uint32_t max_id) {
    if (n < 0) return fail(PPP_ERR_INVALID_ARG, "n must be >= 0");
    if (n >= (1ll << 31)) return fail(PPP_ERR_UNSUPPORTED, "volumes of 2^31 voxels or more are not supported");
    return (int64_t)ppp::post_compact_workspace_bytes(max_id);
}

int ppp_post_compact_ids(uint32_t *d_ids, int64_t n, uint32_t max_id, int64_t compsize, int32_t relabel,
                         uint32_t start, int64_t *n_kept, void *d_work, void *stream) {
    if (n < 0) return fail(PPP_ERR_INVALID_ARG, "n must be >= 0");
    if (n >= (1ll << 31)) return fail(PPP_ERR_UNSUPPORTED, "volumes of 2^31 voxels or more are not supported");
    if (!n_kept || !d_work || (n > 0 && !d_ids) || ((uintptr_t)d_ids & 3))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    long long kept = 0;
    hipError_t e = ppp::run_post_compact(d_ids, n, max_id, compsize, relabel, start, &kept, d_work, (hipStream_t)stream);
    *n_kept = kept;
    if (e == hipErrorInvalidValue) return fail(PPP_ERR_INVALID_ARG, "ppp_post_compact_ids: the map holds an id above max_id");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_post_compact_ids");
}

int64_t ppp_post_dilate_workspace_bytes(int32_t Z, int32_t Y, int32_t X) {
    long long V;
    int rc = post_volume(Z, Y, X, &V);
    return rc != PPP_OK ? rc : (int64_t)ppp::post_dilate_workspace_bytes(V);
}

int ppp_post_dilate(const uint32_t *d_in, uint32_t *d_out, int32_t Z, int32_t Y, int32_t X, int32_t *rounds,
                    void *d_work, void *stream) {
    long long V;
    PPP_TRY(post_volume(Z, Y, X, &V));
    if (!d_in || !d_out || !d_work || !rounds) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (d_in == d_out) return fail(PPP_ERR_INVALID_ARG, "ppp_post_dilate does not work in place");
    PPP_TRY(need_device());
    int r = 0;
    hipError_t e = ppp::run_post_dilate(d_in, d_out, Z, Y, X, &r, d_work, (hipStream_t)stream);
    *rounds = r;
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_post_dilate");
}

int64_t ppp_post_clean_mask_workspace_bytes(int32_t Z, int32_t Y, int32_t X) {
    long long V;
    int rc = post_volume(Z, Y, X, &V);
    return rc != PPP_OK ? rc : (int64_t)ppp::post_clean_mask_workspace_bytes(V);
}

int ppp_post_clean_mask(const uint8_t *d_mask, uint8_t *d_out, int32_t Z, int32_t Y, int32_t X, uint32_t structure,
                        int64_t size, int64_t *n_found, int64_t *n_kept, void *d_work, void *stream) {
    long long V;
    PPP_TRY(post_volume(Z, Y, X, &V));
    if (!d_mask || !d_out || !d_work || !n_found || !n_kept) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    if (structure >> 27) return fail(PPP_ERR_INVALID_ARG, "the structure has 27 bits");
    for (int b = 0; b < 13; ++b)
        if (((structure >> b) & 1u) != ((structure >> (26 - b)) & 1u))
            return fail(PPP_ERR_INVALID_ARG, "the structure must be centrosymmetric");
    PPP_TRY(need_device());
    long long found = 0, kept = 0;
    hipError_t e = ppp::run_post_clean_mask(d_mask, d_out, Z, Y, X, structure, size, &found, &kept, d_work,
                                            (hipStream_t)stream);
    *n_found = found;
    *n_kept = kept;
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_post_clean_mask");
}

/* ---- exact squared distance transform (ppp_edt.hip) and postprocess_fg (ppp_postprocess.hip) ---- */
static int edt_volume(int32_t Z, int32_t Y, int32_t X, long long *V) {
    PPP_TRY(post_volume(Z, Y, X, V));
    // the largest squared distance of the volume must stay below the 32-bit infinity
    if ((long long)Z * Z + (long long)Y * Y + (long long)X * X >= 0xFFFFFFFFll)
        return fail(PPP_ERR_UNSUPPORTED, "squared distances of a %d x %d x %d volume do not fit 32 bits", Z, Y, X);
    return PPP_OK;
}

int64_t ppp_post_edt_sq_workspace_bytes(int32_t Z, int32_t Y, int32_t X) {
    long long V;
    int rc = edt_volume(Z, Y, X, &V);
    return rc != PPP_OK ? rc : (int64_t)ppp::post_edt_workspace_bytes(V);
}

int ppp_post_edt_sq(const uint8_t *d_feature, uint32_t *d_out, int32_t Z, int32_t Y, int32_t X, uint32_t cap,
                    void *d_work, void *stream) {
    long long V;
    PPP_TRY(edt_volume(Z, Y, X, &V));
    if (!d_feature || !d_out || !d_work || ((uintptr_t)d_out & 3)) return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_post_edt_sq(d_feature, d_out, Z, Y, X, cap, d_work, (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_post_edt_sq");
}

int64_t ppp_post_fg_filter_workspace_bytes(int32_t Z, int32_t Y, int32_t X) {
    long long V;
    int rc = edt_volume(Z, Y, X, &V);
    return rc != PPP_OK ? rc : (int64_t)ppp::post_fg_filter_workspace_bytes(V);
}

int ppp_post_fg_filter(const uint8_t *d_mask, uint8_t *d_fg, uint32_t *d_inst, int32_t Z, int32_t Y, int32_t X,
                       int64_t compsize, uint32_t min_d2, int64_t *stats, void *d_work, void *stream) {
    long long V;
    PPP_TRY(edt_volume(Z, Y, X, &V));
    if (!d_mask || !d_fg || !d_work || !stats || ((uintptr_t)d_inst & 3))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    long long st[4] = {0, 0, 0, 0};
    hipError_t e = ppp::run_post_fg_filter(d_mask, d_fg, d_inst, Z, Y, X, compsize, min_d2, st, d_work, (hipStream_t)stream);
    for (int i = 0; i < 4; ++i) stats[i] = st[i];
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_post_fg_filter");
}

/* ---- evaluate_patch (ppp_eval.hip) ---- */
static int eval_args(int32_t L, const int32_t *vol, const int32_t *patch, int32_t z0, int32_t tz, long long *n) {
    if (!vol || !patch) return fail(PPP_ERR_INVALID_ARG, "NULL vol / patch");
    long long V;
    PPP_TRY(post_volume(vol[0], vol[1], vol[2], &V));
    if (L < 1) return fail(PPP_ERR_INVALID_ARG, "labels need at least one channel (L = %d)", L);
    for (int a = 0; a < 3; ++a)
        if (patch[a] < 1 || patch[a] % 2 == 0) return fail(PPP_ERR_INVALID_ARG, "patch side %d must be odd and positive", patch[a]);
    if ((long long)patch[0] * patch[1] * patch[2] > 65535)
        return fail(PPP_ERR_UNSUPPORTED, "patches of more than 65535 elements are not supported");
    if (z0 < 0 || tz < 1 || (long long)z0 + tz > vol[0])
        return fail(PPP_ERR_INVALID_ARG, "z-tile [%d, %d + %d) outside the volume of %d slices", z0, z0, tz, vol[0]);
    *n = (long long)tz * vol[1] * vol[2];
    return PPP_OK;
}

int32_t ppp_eval_patch_thresholds_per_pass(void) { return ppp::kEvalT; }
int32_t ppp_eval_patch_max_thresholds(void) { return ppp::kEvalMaxT; }

int64_t ppp_eval_patch_workspace_bytes(const int32_t *vol, int32_t tz) {
    const int32_t unit[3] = {1, 1, 1};
    long long n;
    int rc = eval_args(1, vol, unit, 0, tz, &n);
    return rc != PPP_OK ? rc : (int64_t)ppp::eval_patch_workspace_bytes(n);
}

int ppp_eval_patch(const void *d_pred, int pred_dtype, int32_t C, const int32_t *d_labels, int32_t L, const int32_t *vol,
                   const int32_t *patch, int32_t z0, int32_t tz, const float *thresholds, int32_t T, int64_t *d_counts,
                   int32_t *d_inter, int32_t *d_union, void *d_work, void *stream) {
    long long n;
    PPP_TRY(eval_args(L, vol, patch, z0, tz, &n));
    PPP_TRY(check_dtype(pred_dtype));
    if (C != patch[0] * patch[1] * patch[2])
        return fail(PPP_ERR_INVALID_ARG, "%d channels, but the patch %d x %d x %d has %d elements", C, patch[0], patch[1],
                    patch[2], patch[0] * patch[1] * patch[2]);
    if (!thresholds || T < 1 || T > ppp::kEvalMaxT) return fail(PPP_ERR_INVALID_ARG, "T = %d thresholds: 1 .. %d", T, ppp::kEvalMaxT);
    for (int t = 0; t < T; ++t)
        if (!(thresholds[t] - thresholds[t] == 0.0f)) return fail(PPP_ERR_INVALID_ARG, "threshold %d is not finite", t);
    if ((d_inter == nullptr) != (d_union == nullptr)) return fail(PPP_ERR_INVALID_ARG, "d_inter and d_union: both or neither");
    if (!d_pred || !d_labels || !d_counts || !d_work || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_labels & 3) ||
        ((uintptr_t)d_inter & 3) || ((uintptr_t)d_union & 3) || ((uintptr_t)d_pred & (pred_dtype == PPP_F32 ? 3 : 1)))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_eval_patch(d_pred, pred_dtype, d_labels, L, vol[0], vol[1], vol[2], patch[0], patch[1], patch[2],
                                       z0, tz, thresholds, T, (long long *)d_counts, d_inter, d_union, d_work,
                                       (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_eval_patch");
}

/* ---- 3-d thinning of the foreground (ppp_skeleton.hip) ---- */
static int skeleton_volume(int32_t Z, int32_t Y, int32_t X) {
    long long V;
    PPP_TRY(post_volume(Z, Y, X, &V));
    // one workgroup row per slice and per four rows of a slice
    if (Z > 65535 || Y > 4 * 65535)
        return fail(PPP_ERR_UNSUPPORTED, "ppp_skeletonize_3d: at most 65535 slices of at most 262140 rows");
    return PPP_OK;
}

int64_t ppp_skeletonize_3d_workspace_bytes(int32_t Z, int32_t Y, int32_t X) {
    int rc = skeleton_volume(Z, Y, X);
    return rc != PPP_OK ? rc : (int64_t)ppp::skeleton_workspace_bytes(Z, Y, X);
}

int ppp_skeletonize_3d(const uint8_t *d_mask, uint8_t *d_out, int32_t Z, int32_t Y, int32_t X, int64_t *n_kept,
                       int32_t *stats, void *d_work, void *stream) {
    PPP_TRY(skeleton_volume(Z, Y, X));
    if (!d_mask || !d_out || !d_work || !n_kept || !stats) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    long long kept = 0;
    int st[3] = {0, 0, 0};
    hipError_t e = ppp::run_skeletonize_3d(d_mask, d_out, Z, Y, X, &kept, st, d_work, (hipStream_t)stream);
    *n_kept = kept;
    stats[0] = st[0]; stats[1] = st[1]; stats[2] = st[2];
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_skeletonize_3d");
}

int64_t ppp_skeletonize_labels_workspace_bytes(int32_t Z, int32_t Y, int32_t X) {
    int rc = skeleton_volume(Z, Y, X);
    return rc != PPP_OK ? rc : (int64_t)ppp::skeleton_labels_workspace_bytes(Z, Y, X);
}

int ppp_skeletonize_labels(const uint32_t *d_labels, uint32_t *d_out, int32_t Z, int32_t Y, int32_t X, int64_t *n_kept,
                           int32_t *stats, void *d_work, void *stream) {
    PPP_TRY(skeleton_volume(Z, Y, X));
    if (!d_labels || !d_out || !d_work || !n_kept || !stats) return fail(PPP_ERR_INVALID_ARG, "NULL pointer argument");
    PPP_TRY(need_device());
    long long kept = 0;
    int st[3] = {0, 0, 0};
    hipError_t e = ppp::run_skeletonize_labels(d_labels, d_out, Z, Y, X, &kept, st, d_work, (hipStream_t)stream);
    *n_kept = kept;
    stats[0] = st[0]; stats[1] = st[1]; stats[2] = st[2];
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_skeletonize_labels");
}

/* ---- the contingency table of two label stacks (ppp_overlap.hip) ---- */
static int overlap_args(int32_t La, int32_t Lb, int32_t Z, int32_t Y, int32_t X, long long *V, long long *streams) {
    if (La < 1 || Lb < 1) return fail(PPP_ERR_INVALID_ARG, "both stacks need at least one channel (La = %d, Lb = %d)", La, Lb);
    PPP_TRY(post_volume(Z, Y, X, V));
    *streams = (long long)La * Lb + La + Lb;
    if (*streams > 65535)
        return fail(PPP_ERR_UNSUPPORTED, "ppp_label_overlap: La Lb + La + Lb = %lld, more than 65535, is not supported", *streams);
    return PPP_OK;
}

int32_t ppp_label_overlap_table_entries(void) { return ppp::overlap_table_entries(); }
uint32_t ppp_label_overlap_slot(uint32_t a, uint32_t b) { return ppp::overlap_slot_host(a, b); }
void ppp_label_overlap_last_stats(int64_t *stats) {
    long long st[3];
    ppp::overlap_last_stats(st);
    if (stats) for (int i = 0; i < 3; ++i) stats[i] = st[i];
}

int64_t ppp_label_overlap_workspace_bytes(int32_t La, int32_t Lb, int32_t Z, int32_t Y, int32_t X) {
    long long V, streams;
    int rc = overlap_args(La, Lb, Z, Y, X, &V, &streams);
    return rc != PPP_OK ? rc : (int64_t)ppp::label_overlap_workspace_bytes(V, streams);
}

int ppp_label_overlap(const uint32_t *d_a, int32_t La, const uint32_t *d_b, int32_t Lb, int32_t Z, int32_t Y, int32_t X,
                      uint32_t *d_rows, int64_t *d_counts, int64_t cap, int64_t *n_rows, void *d_work, void *stream) {
    long long V, streams;
    PPP_TRY(overlap_args(La, Lb, Z, Y, X, &V, &streams));
    if (cap < 0) return fail(PPP_ERR_INVALID_ARG, "cap must be >= 0");
    if (!d_a || !d_b || !n_rows || !d_work || (cap > 0 && (!d_rows || !d_counts)) || ((uintptr_t)d_a & 3) ||
        ((uintptr_t)d_b & 3) || ((uintptr_t)d_rows & 3) || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_work & 7))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    long long n = 0;
    hipError_t e = ppp::run_label_overlap(d_a, La, d_b, Lb, V, d_rows, (long long *)d_counts, cap, &n, d_work,
                                          (hipStream_t)stream);
    *n_rows = n;
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_label_overlap");
}

/* ---- the patch mosaic of visualize_patches (ppp_mosaic.hip) ---- */
int ppp_patch_mosaic(const void *d_pred, int pred_dtype, int32_t C, const uint8_t *d_selected, int32_t S, void *d_out,
                     int32_t tz, int32_t Y, int32_t X, const int32_t *patch, void *stream) {
    if (!patch) return fail(PPP_ERR_INVALID_ARG, "NULL patch");
    if (tz <= 0 || Y <= 0 || X <= 0) return fail(PPP_ERR_INVALID_ARG, "bad z-tile %d x %d x %d", tz, Y, X);
    for (int a = 0; a < 3; ++a)
        if (patch[a] < 1) return fail(PPP_ERR_INVALID_ARG, "patch side %d must be positive", patch[a]);
    PPP_TRY(check_dtype(pred_dtype));
    if ((long long)C != (long long)patch[0] * patch[1] * patch[2])
        return fail(PPP_ERR_INVALID_ARG, "%d channels, but the patch %d x %d x %d has %lld elements", C, patch[0], patch[1],
                    patch[2], (long long)patch[0] * patch[1] * patch[2]);
    if (S != 0 && S != 1 && S != 3) return fail(PPP_ERR_INVALID_ARG, "selected has %d channels: 0, 1 or 3", S);
    if (S > 0 && patch[0] > 1) return fail(PPP_ERR_INVALID_ARG, "selected goes with the 2-d mosaic only (pz = %d)", patch[0]);
    const char *why = "";
    if (!ppp::patch_mosaic_supported(tz, Y, X, patch[0], patch[1], patch[2], &why))
        return fail(PPP_ERR_UNSUPPORTED, "ppp_patch_mosaic: %s are not supported", why);
    if (!d_pred || !d_out || (S > 0) != (d_selected != nullptr) || ((uintptr_t)d_pred & (pred_dtype == PPP_F32 ? 3 : 1)) ||
        ((uintptr_t)d_out & (pred_dtype == PPP_F32 ? 3 : 1)))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_patch_mosaic(d_pred, pred_dtype, d_selected, S, d_out, tz, Y, X, patch[0], patch[1], patch[2],
                                         (hipStream_t)stream);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_mosaic");
}

/* ---- the ground-truth patch affinities as an array (ppp_gt_affs.hip) ---- */
static int gt_affs_labels(int32_t B, int32_t L, const int32_t *vol, int32_t E) {
    if (!vol) return fail(PPP_ERR_INVALID_ARG, "NULL vol");
    if (B < 1 || L < 1) return fail(PPP_ERR_INVALID_ARG, "labels need at least one batch item and one channel (B = %d, L = %d)", B, L);
    long long V;
    PPP_TRY(post_volume(vol[0], vol[1], vol[2], &V));
    if (E < 1) return fail(PPP_ERR_INVALID_ARG, "E = %d: at least one edge", E);
    if (E > 65535) return fail(PPP_ERR_UNSUPPORTED, "E = %d: more than 65535 edges are not supported", E);
    return PPP_OK;
}

static int gt_affs_dense_args(int32_t B, int32_t L, const int32_t *vol, int32_t E, const int32_t *halo, const int32_t *box,
                              int out_dtype, int32_t single) {
    PPP_TRY(gt_affs_labels(B, L, vol, E));
    PPP_TRY(check_dtype(out_dtype));
    if (single && out_dtype != PPP_F32) return fail(PPP_ERR_INVALID_ARG, "the one-channel form (id squared) is float32 only");
    if (single && L != 1) return fail(PPP_ERR_INVALID_ARG, "the one-channel form takes L = 1, not %d", L);
    if (!halo || !box) return fail(PPP_ERR_INVALID_ARG, "NULL halo or box");
    for (int a = 0; a < 3; ++a) {
        if (halo[2 * a] > halo[2 * a + 1])
            return fail(PPP_ERR_INVALID_ARG, "halo of axis %d: minimum %d above maximum %d", a, halo[2 * a], halo[2 * a + 1]);
        if (box[2 * a] < 0 || box[2 * a + 1] > vol[a] || box[2 * a] >= box[2 * a + 1])
            return fail(PPP_ERR_INVALID_ARG, "box [%d, %d) of axis %d is empty or leaves the volume of %d", box[2 * a],
                        box[2 * a + 1], a, vol[a]);
    }
    return PPP_OK;
}

int ppp_gt_affs_dense_plan(int32_t B, int32_t L, const int32_t *vol, int32_t E, const int32_t *halo, const int32_t *box,
                           int out_dtype, int32_t single, int32_t *plan) {
    PPP_TRY(gt_affs_dense_args(B, L, vol, E, halo, box, out_dtype, single));
    if (!plan) return fail(PPP_ERR_INVALID_ARG, "NULL plan");
    ppp::gt_affs_dense_plan(B, L, E, halo, box, plan);
    return PPP_OK;
}

int ppp_gt_affs_dense(const int32_t *d_labels, int32_t B, int32_t L, const int32_t *vol, const int32_t *d_nhood, int32_t E,
                      const int32_t *halo, const int32_t *box, void *d_out, int out_dtype, int32_t single, void *stream) {
    PPP_TRY(gt_affs_dense_args(B, L, vol, E, halo, box, out_dtype, single));
    if (!d_labels || !d_nhood || !d_out || ((uintptr_t)d_labels & 3) || ((uintptr_t)d_nhood & 3) ||
        ((uintptr_t)d_out & (out_dtype == PPP_F32 ? 3 : 1)))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_gt_affs_dense(d_labels, B, L, vol[0], vol[1], vol[2], d_nhood, E, halo, box, d_out, out_dtype,
                                          single ? 1 : 0, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(PPP_ERR_UNSUPPORTED, "ppp_gt_affs_dense: a grid the device would not run whole");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_gt_affs_dense");
}

int ppp_gt_affs_samples(const int32_t *d_labels, int32_t B, int32_t L, const int32_t *vol, const int32_t *d_samples, int64_t N,
                        const int32_t *d_nhood, int32_t E, const int32_t *ps, const int32_t *ctr, void *d_out, int out_dtype,
                        void *stream) {
    PPP_TRY(gt_affs_labels(B, L, vol, E));
    PPP_TRY(check_dtype(out_dtype));
    if (!ps || !ctr) return fail(PPP_ERR_INVALID_ARG, "NULL ps or ctr");
    for (int a = 0; a < 3; ++a)
        if (ps[a] < 1 || ctr[a] < 0 || ctr[a] >= ps[a])
            return fail(PPP_ERR_INVALID_ARG, "axis %d: centre %d outside the patch of %d", a, ctr[a], ps[a]);
    if (N < 0) return fail(PPP_ERR_INVALID_ARG, "N must be >= 0");
    if (N == 0) return PPP_OK;
    if (!d_labels || !d_samples || !d_nhood || !d_out || ((uintptr_t)d_labels & 3) || ((uintptr_t)d_samples & 3) ||
        ((uintptr_t)d_nhood & 3) || ((uintptr_t)d_out & (out_dtype == PPP_F32 ? 3 : 1)))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_gt_affs_samples(d_labels, B, L, vol[0], vol[1], vol[2], d_samples, (long long)N, d_nhood, E, ps, ctr,
                                            d_out, out_dtype, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(PPP_ERR_UNSUPPORTED, "ppp_gt_affs_samples: N = %lld is more than one launch runs", (long long)N);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_gt_affs_samples");
}

/* ---- the fused patch loss from the labels (ppp_patch_loss.hip) ---- */
static int patch_loss_dense_args(int32_t B, int32_t L, const int32_t *vol, int32_t E, const int32_t *halo, const int32_t *box,
                                 int dtype) {
    return gt_affs_dense_args(B, L, vol, E, halo, box, dtype, 0);
}

static int patch_loss_samples_args(int32_t B, int32_t L, const int32_t *vol, int32_t E, const int32_t *ps, const int32_t *ctr,
                                   int dtype, int64_t N) {
    PPP_TRY(gt_affs_labels(B, L, vol, E));
    PPP_TRY(check_dtype(dtype));
    if (!ps || !ctr) return fail(PPP_ERR_INVALID_ARG, "NULL ps or ctr");
    for (int a = 0; a < 3; ++a)
        if (ps[a] < 1 || ctr[a] < 0 || ctr[a] >= ps[a])
            return fail(PPP_ERR_INVALID_ARG, "axis %d: centre %d outside the patch of %d", a, ctr[a], ps[a]);
    if (N < 0) return fail(PPP_ERR_INVALID_ARG, "N must be >= 0");
    return PPP_OK;
}

static bool bad_ptr(const void *p, uintptr_t mask) { return !p || ((uintptr_t)p & mask); }

int64_t ppp_patch_loss_workspace_bytes(int32_t B, int32_t L, const int32_t *vol, int32_t E, const int32_t *halo,
                                       const int32_t *box, int dtype, int64_t N) {
    if (box) {
        int rc = patch_loss_dense_args(B, L, vol, E, halo, box, dtype);
        return rc != PPP_OK ? rc : (int64_t)ppp::patch_loss_workspace_bytes(B, L, E, halo, box, 0);
    }
    int rc = gt_affs_labels(B, L, vol, E);
    if (rc == PPP_OK) rc = check_dtype(dtype);
    if (rc == PPP_OK && N < 0) rc = fail(PPP_ERR_INVALID_ARG, "N must be >= 0");
    return rc != PPP_OK ? rc : (int64_t)ppp::patch_loss_workspace_bytes(B, L, E, nullptr, nullptr, (long long)N);
}

int ppp_patch_loss_dense_fwd(const void *d_logits, int dtype, const int32_t *d_labels, int32_t B, int32_t L, const int32_t *vol,
                             const int32_t *d_nhood, int32_t E, const int32_t *halo, const int32_t *box, const float *d_weight,
                             double num_channels, float *d_loss, double *d_state, int64_t *d_counts, void *d_work, void *stream) {
    PPP_TRY(patch_loss_dense_args(B, L, vol, E, halo, box, dtype));
    if (d_weight && !(num_channels > 0.0 && num_channels <= 1.7e308))
        return fail(PPP_ERR_INVALID_ARG, "num_channels = %g: a positive finite factor", num_channels);
    if (bad_ptr(d_logits, dtype == PPP_F32 ? 3 : 1) || bad_ptr(d_labels, 3) || bad_ptr(d_nhood, 3) || bad_ptr(d_loss, 3) ||
        bad_ptr(d_state, 7) || bad_ptr(d_work, 7) || ((uintptr_t)d_weight & 3) || ((uintptr_t)d_counts & 7))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_patch_loss_dense(true, d_logits, dtype, d_labels, B, L, vol[0], vol[1], vol[2], d_nhood, E, halo, box,
                                             d_weight, num_channels, d_loss, d_state, (long long *)d_counts, nullptr, nullptr,
                                             d_work, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(PPP_ERR_UNSUPPORTED, "ppp_patch_loss_dense_fwd: a grid the device would not run whole");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_loss_dense_fwd");
}

int ppp_patch_loss_dense_bwd(const void *d_logits, int dtype, const int32_t *d_labels, int32_t B, int32_t L, const int32_t *vol,
                             const int32_t *d_nhood, int32_t E, const int32_t *halo, const int32_t *box, const float *d_weight,
                             const double *d_state, const float *d_grad_out, void *d_grad, void *stream) {
    PPP_TRY(patch_loss_dense_args(B, L, vol, E, halo, box, dtype));
    if (bad_ptr(d_logits, dtype == PPP_F32 ? 3 : 1) || bad_ptr(d_labels, 3) || bad_ptr(d_nhood, 3) || bad_ptr(d_state, 7) ||
        bad_ptr(d_grad_out, 3) || bad_ptr(d_grad, dtype == PPP_F32 ? 3 : 1) || ((uintptr_t)d_weight & 3))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_patch_loss_dense(false, d_logits, dtype, d_labels, B, L, vol[0], vol[1], vol[2], d_nhood, E, halo, box,
                                             d_weight, 0.0, nullptr, const_cast<double *>(d_state), nullptr, d_grad_out, d_grad,
                                             nullptr, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(PPP_ERR_UNSUPPORTED, "ppp_patch_loss_dense_bwd: a grid the device would not run whole");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_loss_dense_bwd");
}

int ppp_patch_loss_samples_fwd(const void *d_logits, int dtype, const int32_t *d_labels, int32_t B, int32_t L, const int32_t *vol,
                               const int32_t *d_samples, int64_t N, const int32_t *d_nhood, int32_t E, const int32_t *ps,
                               const int32_t *ctr, float *d_loss, double *d_state, void *d_work, void *stream) {
    PPP_TRY(patch_loss_samples_args(B, L, vol, E, ps, ctr, dtype, N));
    if (N == 0) return PPP_OK;
    if (bad_ptr(d_logits, dtype == PPP_F32 ? 3 : 1) || bad_ptr(d_labels, 3) || bad_ptr(d_samples, 3) || bad_ptr(d_nhood, 3) ||
        bad_ptr(d_loss, 3) || bad_ptr(d_state, 7) || bad_ptr(d_work, 7))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_patch_loss_samples(true, d_logits, dtype, d_labels, B, L, vol[0], vol[1], vol[2], d_samples, (long long)N,
                                               d_nhood, E, ps, ctr, d_loss, d_state, nullptr, nullptr, d_work, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(PPP_ERR_UNSUPPORTED, "ppp_patch_loss_samples_fwd: N = %lld is more than one launch runs", (long long)N);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_loss_samples_fwd");
}

int ppp_patch_loss_samples_bwd(const void *d_logits, int dtype, const int32_t *d_labels, int32_t B, int32_t L, const int32_t *vol,
                               const int32_t *d_samples, int64_t N, const int32_t *d_nhood, int32_t E, const int32_t *ps,
                               const int32_t *ctr, const double *d_state, const float *d_grad_out, void *d_grad, void *stream) {
    PPP_TRY(patch_loss_samples_args(B, L, vol, E, ps, ctr, dtype, N));
    if (N == 0) return PPP_OK;
    if (bad_ptr(d_logits, dtype == PPP_F32 ? 3 : 1) || bad_ptr(d_labels, 3) || bad_ptr(d_samples, 3) || bad_ptr(d_nhood, 3) ||
        bad_ptr(d_state, 7) || bad_ptr(d_grad_out, 3) || bad_ptr(d_grad, dtype == PPP_F32 ? 3 : 1))
        return fail(PPP_ERR_INVALID_ARG, "NULL or misaligned pointer argument");
    PPP_TRY(need_device());
    hipError_t e = ppp::run_patch_loss_samples(false, d_logits, dtype, d_labels, B, L, vol[0], vol[1], vol[2], d_samples, (long long)N,
                                               d_nhood, E, ps, ctr, nullptr, const_cast<double *>(d_state), d_grad_out, d_grad,
                                               nullptr, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(PPP_ERR_UNSUPPORTED, "ppp_patch_loss_samples_bwd: N = %lld is more than one launch runs", (long long)N);
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_patch_loss_samples_bwd");
}

/* ---- a stored chunk to its place in a device tensor (ppp_chunk.hip) ---- */
int ppp_chunk_scatter(const void *d_src, int64_t nbytes, int32_t typesize, int64_t blocksize, int32_t shuffle,
                      int32_t ndim, const int64_t *chunk_shape, const int64_t *chunk_origin,
                      const int64_t *sel_lo, const int64_t *sel_hi, void *d_dst,
                      int32_t flags_dtype, int32_t *d_flags, void *stream) {
    if (typesize != 1 && typesize != 2 && typesize != 4)
        return fail(PPP_ERR_UNSUPPORTED, "ppp_chunk_scatter: elements of %d bytes (1, 2 and 4 are served)", typesize);
    if (ndim > 4) return fail(PPP_ERR_UNSUPPORTED, "ppp_chunk_scatter: %d axes (up to 4 are served)", ndim);
    if (ndim < 1 || !chunk_shape || !chunk_origin || !sel_lo || !sel_hi || nbytes < 0)
        return fail(PPP_ERR_INVALID_ARG, "ppp_chunk_scatter: bad argument");
    if (shuffle != PPP_SHUFFLE_NONE && shuffle != PPP_SHUFFLE_BYTE && shuffle != PPP_SHUFFLE_BIT)
        return fail(PPP_ERR_INVALID_ARG, "ppp_chunk_scatter: bad shuffle kind %d", shuffle);
    if (shuffle == PPP_SHUFFLE_NONE) blocksize = 1 << 22;       // no block structure: any split serves
    if (blocksize <= 0 || blocksize > (1ll << 30) || blocksize % typesize)
        return fail(PPP_ERR_INVALID_ARG, "ppp_chunk_scatter: blocksize %lld must be a multiple of the element size, at most 2^30",
                    (long long)blocksize);
    if (d_flags && !((flags_dtype == PPP_F16 && typesize == 2) || (flags_dtype == PPP_F32 && typesize == 4)))
        return fail(PPP_ERR_INVALID_ARG, "ppp_chunk_scatter: flags are for float16 (2 bytes) and float32 (4 bytes) elements");
    ppp::ChunkGeo g;
    memset(&g, 0, sizeof(g));
    const int pad = 4 - ndim;
    long long count = 1, extent[4] = {1, 1, 1, 1}, first = 0;
    bool empty = false;
    for (int a = 0; a < 4; ++a) g.cs[a] = 1, g.clo[a] = 0, g.chi[a] = 1;
    for (int i = 0; i < ndim; ++i) {
        const int a = pad + i;
        if (chunk_shape[i] <= 0 || chunk_shape[i] > 0x7fffffffll || sel_hi[i] < sel_lo[i] || chunk_origin[i] < 0 || sel_lo[i] < 0)
            return fail(PPP_ERR_INVALID_ARG, "ppp_chunk_scatter: bad extent on axis %d", i);
        count *= chunk_shape[i];
        if (count > (1ll << 40)) return fail(PPP_ERR_INVALID_ARG, "ppp_chunk_scatter: chunk too large");
        g.cs[a] = (int)chunk_shape[i];
        const long long lo = sel_lo[i] > chunk_origin[i] ? sel_lo[i] - chunk_origin[i] : 0;
        const long long hi = sel_hi[i] - chunk_origin[i] < chunk_shape[i] ? sel_hi[i] - chunk_origin[i] : chunk_shape[i];
        if (hi <= lo) empty = true;
        g.clo[a] = (int)lo;
        g.chi[a] = (int)(hi > lo ? hi : lo);
        extent[a] = sel_hi[i] - sel_lo[i];
    }
    if (count * typesize != nbytes)
        return fail(PPP_ERR_INVALID_ARG, "ppp_chunk_scatter: %lld bytes are not a chunk of %lld elements of %d bytes",
                    (long long)nbytes, count, typesize);
    if (empty || nbytes == 0) return PPP_OK;
    if (!d_src || !d_dst || ((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & (uintptr_t)(typesize - 1)))
        return fail(PPP_ERR_INVALID_ARG, "ppp_chunk_scatter: NULL or misaligned pointer argument");
    // destination strides (elements) and the element the chunk coordinate clo lands on
    long long stride[4];
    stride[3] = 1;
    for (int a = 2; a >= 0; --a) stride[a] = stride[a + 1] * extent[a + 1];
    for (int a = 0; a < 4; ++a) {
        const long long org = a >= pad ? chunk_origin[a - pad] - sel_lo[a - pad] : 0;
        first += (org + g.clo[a]) * stride[a];
        if (a < 3) g.dstride[a] = stride[a];
    }
    g.src = (const uint8_t *)d_src;
    g.nbytes = nbytes;
    g.blocksize = blocksize;
    g.shuffle = shuffle;
    g.dst = (char *)d_dst + first * typesize;
    g.fkind = d_flags ? flags_dtype : -1;
    g.flags = d_flags;
    PPP_TRY(need_device());
    hipError_t e = ppp::launch_chunk_scatter(g, typesize, (hipStream_t)stream);
    if (e == hipErrorInvalidConfiguration) return fail(PPP_ERR_UNSUPPORTED, "ppp_chunk_scatter: the chunk is more than one launch runs");
    return e == hipSuccess ? PPP_OK : hip_fail(e, "ppp_chunk_scatter");
}

}  // extern "C"
