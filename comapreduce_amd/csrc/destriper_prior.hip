// destriper_prior.hip -- a noise prior on the destriper's offsets: the banded C_a^-1 term of
// (A + T) x = b (MADAM's F^T W Z F + C_a^-1) on a one-band problem built by destriper_setup.hip.
//
// Offsets are taken in the CALLER's (time) order.  Every offset carries a group id in [-1, G); group
// g occupies one contiguous run [s_g, e_g) of offsets and has a stencil t_g[0 .. K], 1 <= K <= 64.  T
// is block diagonal: group g's block is the (e_g - s_g)-square finite section of the symmetric banded
// Toeplitz matrix with first row t_g.  An offset with id -1 has no prior (a zero row and column).
//
// y = T v in a fixed order, every product and every sum rounded to f64 on its own:
//     y_i = t_g[0] v_i;   for k = 1 .. K:   if i - k >= s_g: y_i += t_g[k] v_{i-k}
//                                           if i + k <  e_g: y_i += t_g[k] v_{i+k}
// and y_i = +0.0 for id -1 (destriper.prior_apply_reference restates it in NumPy, bit for bit).
//
// The problem's vectors are in its internal (spatially sorted) offset order, so the kernel gathers
// through the inverse of d->perm: one workgroup takes kPriorTile consecutive caller-order offsets,
// stages v for the tile and a halo of K on each side in LDS (coalesced index loads, a gathered value
// each), and one lane computes one offset.  A lane needs only its own group's bounds, which it keeps
// in registers.  No atomics; two calls agree bit for bit.
//
// comap_destripe_prior_solve (end of this file) is comap_destripe_solve's CG on (A + T): the same
// four launches per iteration plus this kernel, which adds T p to q and leaves its block partials of
// p . (T p) behind the projection's p . (A p) partials in d->part, where the fused update sums them.
// The eager driver (Python's cg_solve on PriorOps) gets the same two parts through
// comap_destripe_project's own dot and comap_destripe_prior_apply_dot.
#include "destriper_internal.h"

// every product below is rounded before it is added (hipcc contracts a * b + c by default)
#pragma clang fp contract(off)

constexpr int kPriorTile = 256;      // caller-order offsets per workgroup sweep (= its threads)
constexpr int kPriorMaxK = 64;       // stencil half-width bound (the halo staged on each side)
constexpr int kPriorBlocks = 2048;   // apply grid cap: its partials follow the projection's in d->part

struct comap_prior {
    comap_destriper *d = nullptr;
    comap_ctx *ctx = nullptr;
    int64_t NO = 0, G = 0;
    int32_t K = 0;
    int32_t *gid = nullptr;      // [NO] group of caller-order offset i (-1: none)
    int32_t *bounds = nullptr;   // [2 G] s_g, e_g (0, 0 for a group without offsets)
    double *stencil = nullptr;   // [G][K + 1]
    int32_t *inv = nullptr;      // [NO] caller's offset -> internal position (inverse of d->perm)
    // device-resident CG of comap_destripe_prior_solve (fixed pointers: graph-replayable); the stream,
    // scalars, stop flags and partials are the plain problem's (d->cs, scal, flags, part)
    double *cg = nullptr;        // [4 NO + npix]: x, r, p, q | num
    hipGraphExec_t batch = nullptr;   // kCgBatch iterations
};

namespace {

// inv[perm[k]] = k
__global__ void k_pr_invert(const int32_t *__restrict__ perm, int64_t NO, int32_t *__restrict__ inv)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < NO; k += (int64_t)gridDim.x * blockDim.x)
        inv[perm[k]] = (int32_t)k;
}

// The runs of equal id: a run of group g starts at i when gid[i - 1] != g and ends behind i when
// gid[i + 1] != g.  runs[g] counts the starts (an integer count: no order to keep); bounds[2g],
// bounds[2g + 1] = the run (any of them when there are several, which k_pr_runs then rejects).
// flag[0]: an id outside [-1, G).
__global__ void k_pr_scan(const int32_t *__restrict__ gid, int64_t NO, int64_t G, int32_t *__restrict__ runs,
                          int32_t *__restrict__ bounds, int32_t *__restrict__ flag)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < NO; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t g = gid[i];
        if (g < -1 || g >= G) { flag[0] = 1; continue; }
        if (g < 0) continue;
        if (i == 0 || gid[i - 1] != g) {
            atomicAdd(&runs[g], 1);
            bounds[2 * g] = (int32_t)i;
        }
        if (i == NO - 1 || gid[i + 1] != g) bounds[2 * g + 1] = (int32_t)(i + 1);
    }
}

// flag[1]: a group in more than one run
__global__ void k_pr_runs(const int32_t *__restrict__ runs, int64_t G, int32_t *__restrict__ flag)
{
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x)
        if (runs[g] > 1) flag[1] = 1;
}

// out = T v (ACC: out += T v), v and out in the internal order; part != NULL: this block's partial
// of v . (T v) in part[blockIdx.x] (lane-strided over its tiles, then the block: a fixed order).
// flags: the native solve's stop flags (NULL for the per-piece call).
template <bool ACC>
__global__ void __launch_bounds__(kPriorTile) k_pr_apply(const int32_t *__restrict__ gid,
                                                         const int32_t *__restrict__ bounds,
                                                         const double *__restrict__ stencil, int K,
                                                         const int32_t *__restrict__ inv, const double *__restrict__ v,
                                                         double *__restrict__ out, int64_t NO,
                                                         double *__restrict__ part, const int32_t *__restrict__ flags)
{
    __shared__ double sv[kPriorTile + 2 * kPriorMaxK];
    __shared__ double red[4];
    if (flags && flags[0]) return;
    const int tid = threadIdx.x;
    const int64_t ntiles = (NO + kPriorTile - 1) / kPriorTile;
    double acc = 0.0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * kPriorTile;
        __syncthreads();   // (the previous tile's reads of sv are done)
        for (int j = tid; j < kPriorTile + 2 * K; j += kPriorTile) {
            const int64_t c = base - K + j;
            sv[j] = (c >= 0 && c < NO) ? v[inv[c]] : 0.0;
        }
        __syncthreads();
        const int64_t i = base + tid;
        if (i < NO) {
            const int32_t g = gid[i];
            const double *c = sv + K + tid;   // c[k] = v of caller-order offset i + k
            double y = 0.0;
            if (g >= 0) {
                const int64_t s = bounds[2 * g], e = bounds[2 * g + 1];
                const double *t = stencil + (int64_t)g * (K + 1);
                y = t[0] * c[0];
                for (int k = 1; k <= K; ++k) {
                    const double tk = t[k];
                    if (i - k >= s) y += tk * c[-k];
                    if (i + k < e) y += tk * c[k];
                }
            }
            const int32_t o = inv[i];
            if constexpr (ACC) out[o] = out[o] + y;
            else out[o] = y;
            acc += c[0] * y;
        }
    }
    if (part) {
        acc = wave_sum(acc);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// dot[0] += the fixed-order sum of the apply kernel's n block partials (k_dot_final's order)
__global__ void __launch_bounds__(256) k_pr_dot_add(const double *__restrict__ part, int n, double *__restrict__ dot)
{
    __shared__ double red[4];
    const double s = block_final_sum(part, n, red);
    if (threadIdx.x == 0) dot[0] = dot[0] + s;
}

unsigned prior_grid(int64_t NO, int64_t cap = kPriorBlocks)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((NO + kPriorTile - 1) / kPriorTile, cap));
}

void launch_apply(const comap_prior *pr, hipStream_t st, unsigned grid, const double *v, double *out, bool accumulate,
                  double *part, const int32_t *flags)
{
    if (accumulate)
        k_pr_apply<true><<<grid, kPriorTile, 0, st>>>(pr->gid, pr->bounds, pr->stencil, pr->K, pr->inv, v, out, pr->NO,
                                                      part, flags);
    else
        k_pr_apply<false><<<grid, kPriorTile, 0, st>>>(pr->gid, pr->bounds, pr->stencil, pr->K, pr->inv, v, out, pr->NO,
                                                       part, flags);
}

void prior_free(comap_prior *pr, bool idle)
{
    if (pr->batch) (void)hipGraphExecDestroy(pr->batch);
    void *b[] = {pr->gid, pr->bounds, pr->stencil, pr->inv, pr->cg};
    comap_tmp_free_on(b, (int)(sizeof(b) / sizeof(b[0])), nullptr, idle);
    delete pr;
}

int prior_build(comap_prior *pr, const int32_t *gid, const double *stencil)
{
    comap_destriper *d = pr->d;
    comap_ctx *ctx = pr->ctx;
    hipStream_t st = ctx->stream;
    const int64_t NO = pr->NO, G = pr->G;
    int rc = 0;
    rc |= dalloc(ctx, &pr->gid, NO);
    rc |= dalloc(ctx, &pr->bounds, 2 * G);
    rc |= dalloc(ctx, &pr->stencil, G * (pr->K + 1));
    rc |= dalloc(ctx, &pr->inv, NO);
    if (rc) return -2;
    DevTemps tmp(st);
    int32_t *runs = nullptr, *flag = nullptr;
    COMAP_CHECK(ctx, tmp.alloc(&runs, G));
    COMAP_CHECK(ctx, tmp.alloc(&flag, 2));
    COMAP_CHECK(ctx, hipMemcpyAsync(pr->gid, gid, 4 * (size_t)NO, hipMemcpyDeviceToDevice, st));
    COMAP_CHECK(ctx, hipMemcpyAsync(pr->stencil, stencil, 8 * (size_t)(G * (pr->K + 1)), hipMemcpyDeviceToDevice, st));
    COMAP_CHECK(ctx, hipMemsetAsync(runs, 0, 4 * (size_t)G, st));
    COMAP_CHECK(ctx, hipMemsetAsync(pr->bounds, 0, 8 * (size_t)G, st));
    COMAP_CHECK(ctx, hipMemsetAsync(flag, 0, 8, st));
    k_pr_invert<<<grid_for(NO), 256, 0, st>>>(d->perm, NO, pr->inv);
    k_pr_scan<<<grid_for(NO), 256, 0, st>>>(pr->gid, NO, G, runs, pr->bounds, flag);
    k_pr_runs<<<grid_for(G), 256, 0, st>>>(runs, G, flag);
    COMAP_LAUNCH_CHECK(ctx);
    int32_t hf[2] = {0, 0};
    COMAP_CHECK(ctx, hipMemcpyAsync(hf, flag, 8, hipMemcpyDeviceToHost, st));
    COMAP_CHECK(ctx, hipStreamSynchronize(st));
    if (hf[0]) return comap_fail(ctx, -3, "noise prior: group id out of range (valid: -1 .. n_groups - 1)");
    if (hf[1]) return comap_fail(ctx, -3, "noise prior: a group id occupies more than one run of offsets");
    return 0;
}

}  // namespace

extern "C" int32_t comap_destripe_prior_tile(void) { return kPriorTile; }

extern "C" int comap_destripe_prior_create(comap_destriper *d, const int32_t *gid, int64_t n_groups, const double *stencil,
                                           int32_t K, comap_prior **out)
{
    if (!d || !out) return -1;
    comap_ctx *ctx = d->ctx;
    if (!gid || !stencil) return comap_fail(ctx, -1, "noise prior: null input");
    if (d->nb != 1) return comap_fail(ctx, -1, "noise prior: one band per problem (batched bands are not supported)");
    if (K < 1 || K > kPriorMaxK) return comap_fail(ctx, -3, "noise prior: stencil half-width K must lie in 1 .. 64");
    if (n_groups < 1 || n_groups > (1 << 24)) return comap_fail(ctx, -3, "noise prior: 1 .. 2^24 groups");
    if (d->NO >= (int64_t(1) << 31)) return comap_fail(ctx, -1, "noise prior: the offset count must fit 31 bits");
    COMAP_DEVICE_GUARD(ctx);
    comap_prior *pr = new comap_prior;
    pr->d = d;
    pr->ctx = ctx;
    pr->NO = d->NO;
    pr->G = n_groups;
    pr->K = K;
    const int rc = prior_build(pr, gid, stencil);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        prior_free(pr, true);
        return rc;
    }
    *out = pr;
    return 0;
}

extern "C" int comap_destripe_prior_destroy(comap_prior *pr)
{
    if (!pr) return 0;
    COMAP_DEVICE_GUARD(pr->ctx);
    (void)hipDeviceSynchronize();
    prior_free(pr, true);
    return 0;
}

extern "C" int comap_destripe_prior_apply(comap_prior *pr, const double *v, double *out, int32_t accumulate)
{
    if (!pr || !v || !out || v == out) return -1;
    COMAP_DEVICE_GUARD(pr->ctx);
    comap_ctx *ctx = pr->ctx;
    launch_apply(pr, ctx->stream, prior_grid(pr->NO), v, out, accumulate != 0, nullptr, nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

// apply, then dot[0] += v . (T v): the eager driver's p . q is comap_destripe_project's own p . (A p)
// with the prior's part added, so a zero prior leaves every bit of the plain solve in place.  The
// block partials pass through d->part, behind whatever the stream ran before.
extern "C" int comap_destripe_prior_apply_dot(comap_prior *pr, const double *v, double *out, int32_t accumulate,
                                              double *dot)
{
    if (!pr || !v || !out || !dot || v == out) return -1;
    COMAP_DEVICE_GUARD(pr->ctx);
    comap_ctx *ctx = pr->ctx;
    const unsigned ng = prior_grid(pr->NO);
    launch_apply(pr, ctx->stream, ng, v, out, accumulate != 0, pr->d->part, nullptr);
    k_pr_dot_add<<<1, 256, 0, ctx->stream>>>(pr->d->part, (int)ng, dot);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

// ---------------------------------------------------------------- device-resident CG with the prior
// comap_destripe_solve's iteration on the prior's own vectors: its bin, projection (p . (A p)
// partials in d->part[0, pg)), then q += T p with the p . (T p) partials in d->part[pg, pg + ng), the
// fused update over all pg + ng partials and the fused direction.  5 launches on the one CG stream.
static int prior_enqueue_iteration(comap_prior *pr, hipStream_t st)
{
    comap_destriper *d = pr->d;
    const int64_t NO = pr->NO;
    double *x = pr->cg, *r = x + NO, *p = r + NO, *q = p + NO, *num = q + NO;
    int32_t *flags = d->flags;
    ds_launch_bin(d, st, d->cf ? d->pt : p, nullptr, d->h, num, flags, true, d->cf);   // empty rows of num stay 0
    const unsigned pg = ds_launch_project_parts(d, st, p, num, q, flags);
    if ((int64_t)pg >= kPartMax) return -1;
    const unsigned ng = prior_grid(NO, std::min<int64_t>(kPriorBlocks, kPartMax - (int64_t)pg));
    launch_apply(pr, st, ng, p, q, true, d->part + pg, flags);
    ds_launch_update_fused(d, st, (int)(pg + ng), x, r, p, q, flags);
    ds_launch_direction_fused(d, st, p, r, flags);
    return 0;
}

// CG vectors and (small problems, or COMAP_DS_CGGRAPH=1) the kCgBatch-iteration graph, on first use
static int prior_cg_setup(comap_prior *pr)
{
    comap_destriper *d = pr->d;
    comap_ctx *ctx = pr->ctx;
    if (pr->cg && (pr->batch || !ds_cg_use_graph(d))) return 0;
    if (!pr->cg && dalloc(ctx, &pr->cg, 4 * (size_t)pr->NO + (size_t)d->npix)) return -2;
    if (const int rc = ds_cg_state(d)) return rc;
    if (!ds_cg_use_graph(d)) return 0;
    // (the vectors were allocated in the context stream's order: the capture below only records)
    hipGraph_t gr = nullptr;
    int bad = 0;
    COMAP_CHECK(ctx, hipStreamBeginCapture(d->cs, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < kCgBatch; ++i) bad |= prior_enqueue_iteration(pr, d->cs);
    COMAP_CHECK(ctx, hipStreamEndCapture(d->cs, &gr));
    if (bad) {
        (void)hipGraphDestroy(gr);
        return comap_fail(ctx, -1, "noise prior: the projection's grid leaves no partial slots");
    }
    const hipError_t e = hipGraphInstantiate(&pr->batch, gr, nullptr, nullptr, 0);
    (void)hipGraphDestroy(gr);
    COMAP_CHECK(ctx, e);
    return 0;
}

// cg_solve(PriorOps, identity, threshold, niter) without Python per iteration: kCgBatch iterations per
// graph launch and host check, a remainder as plain launches; the device stop flag makes the
// iterations queued behind convergence no-ops.  x in the caller's order, then the plain solve's maps.
extern "C" int comap_destripe_prior_solve(comap_prior *pr, double threshold, int32_t niter, double *x_out, double *map,
                                          double *naive, double *weight, double *hits, int32_t *iters_out)
{
    if (!pr || !x_out || niter < 0) return -1;
    COMAP_DEVICE_GUARD(pr->ctx);
    comap_ctx *ctx = pr->ctx;
    comap_destriper *d = pr->d;
    int rc = prior_cg_setup(pr);
    if (rc) return rc;
    hipStream_t st = d->cs;
    const int64_t NO = pr->NO, np = d->npix;
    double *x = pr->cg, *r = x + NO, *p = r + NO, *num = p + 2 * NO;
    // inputs (and the vectors' allocation) are ordered on the caller's stream
    COMAP_CHECK(ctx, hipEventRecord(d->ev, ctx->stream));
    COMAP_CHECK(ctx, hipStreamWaitEvent(st, d->ev, 0));
    d->thr_host[0] = threshold;
    COMAP_CHECK(ctx, hipMemcpyAsync(d->scal + 4, d->thr_host, 8, hipMemcpyHostToDevice, st));
    COMAP_CHECK(ctx, hipMemsetAsync(x, 0, 8 * (size_t)NO, st));
    COMAP_CHECK(ctx, hipMemsetAsync(num, 0, 8 * (size_t)np, st));   // the CG bin writes only the non-empty rows
    COMAP_CHECK(ctx, hipMemsetAsync(d->flags, 0, 4 * 4, st));
    // b has no prior term; r = p = b (x0 = 0); rr = rr0 = b.b
    ds_launch_project(d, st, nullptr, d->nnum, d->h, r, nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    COMAP_CHECK(ctx, hipMemcpyAsync(p, r, 8 * (size_t)NO, hipMemcpyDeviceToDevice, st));
    if (d->cf) ds_scale(d, st, p, d->pt);   // the first bin's input (later ones come from the direction kernel)
    ds_dot(d, st, r, r, NO, d->scal);
    COMAP_LAUNCH_CHECK(ctx);
    COMAP_CHECK(ctx, hipMemcpyAsync(d->scal + 1, d->scal, 8, hipMemcpyDeviceToDevice, st));
    COMAP_CHECK(ctx, hipMemcpyAsync(d->scal + 3, d->scal, 8, hipMemcpyDeviceToDevice, st));   // current rr
    for (int i = 0; i < 4; ++i) d->flags_host[i] = 0;
    for (int enq = 0; enq < niter;) {
        const int k = std::min(kCgBatch, niter - enq);
        if (k == kCgBatch && pr->batch) {
            COMAP_CHECK(ctx, hipGraphLaunch(pr->batch, st));
        } else {
            for (int i = 0; i < k; ++i)
                if (prior_enqueue_iteration(pr, st))
                    return comap_fail(ctx, -1, "noise prior: the projection's grid leaves no partial slots");
            COMAP_LAUNCH_CHECK(ctx);
        }
        enq += k;
        COMAP_CHECK(ctx, hipMemcpyAsync(d->flags_host, d->flags, 4 * 4, hipMemcpyDeviceToHost, st));
        COMAP_CHECK(ctx, hipStreamSynchronize(st));
        if (d->flags_host[0]) break;
    }
    if (iters_out) iters_out[0] = d->flags_host[3];
    ds_unpermute(d, st, x, x_out);
    // final maps: map = (sum w tod - W x) / h ; naive = sum w tod / h -- of a solve-mask view's parent
    // (the full weights) when the prior sits on a view, as comap_destripe_solve_view's
    const comap_destriper *md = d->parent ? d->parent : d;
    if (map) {
        ds_launch_bin(md, st, x, md->nnum, nullptr, num, nullptr, false, false);
        ds_div_map(st, num, md->h, np, map);
    }
    if (naive) ds_div_map(st, md->nnum, md->h, np, naive);
    COMAP_LAUNCH_CHECK(ctx);
    if (weight) COMAP_CHECK(ctx, hipMemcpyAsync(weight, md->h, 8 * (size_t)np, hipMemcpyDeviceToDevice, st));
    if (hits) COMAP_CHECK(ctx, hipMemcpyAsync(hits, md->hits, 8 * (size_t)np, hipMemcpyDeviceToDevice, st));
    COMAP_CHECK(ctx, hipStreamSynchronize(st));
    return 0;
}
