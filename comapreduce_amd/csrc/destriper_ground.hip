// destriper_ground.hip -- the ground (azimuth) template of the destriper's CG: the reference's
// op_Ax_with_ground (MapMaking/Destriper.py:265-336) on a problem built by destriper_setup.hip.
//
// Unknowns [x_0 .. x_{NO-1} | s_0 .. s_{K-1} | c_0 .. c_{K-1}]: one offset per L samples and, per
// group k = (observation, feed), an azimuth slope s_k and a level c_k.  The template of sample t
// (offset o, group k) is x_o + s_k a_t + c_k and the operator is A = [F G]^T W Z [F G] with the
// plain destriper's binning, map division (m_p = num_p where h_p == 0) and m[pointing] wrap.
//
// Two deviations from the reference:
//   1. a_t = (az_t - mu_k) / sigma_k with the plain mean and rms of the group's azimuths (a_t = 0
//      when the group's azimuth is constant): the same model space -- the level absorbs the shift
//      -- with a condition number CG can work with (raw degrees gave eigenvalues of 4.5e6).  The
//      caller converts back: slope = s / sigma, level = c - s mu / sigma.
//   2. every offset lies in ONE group (the caller passes a group id per offset).  The reference
//      selects samples; the aggregated form below needs whole offsets.
//
// Aggregated form.  With g(o) the group of offset o, x'_o = x_o + c_{g(o)} (the level folded into
// the offsets) and, per offset, wa_o = sum w a; per group, Saa_k = sum w a^2, Ta_k = sum w a tod;
// per (group, pixel) entry e, ga_e = sum w a over the group's samples that fall in that pixel:
//     num  = W x' (comap_destripe_bin)  +  sum_{e in pixel row p} ga_e s_{k(e)}     ground_bin
//     y_o  = comap_destripe_project(x', num)  +  wa_o s_{g(o)}                      ground_project
//     z1_k = sum_{o in k} y_o
//     za_k = sum_{o in k} wa_o x'_o + Saa_k s_k - sum_{e in group row k} ga_e m[read pixel of e]
//     rhs:  b1_k = sum_{o in k} b_o,  ba_k = Ta_k - sum_e ga_e m_naive[read pixel of e]
// The plain destriper's kernels are used through their C ABI, unchanged.
//
// Azimuth wrap.  A group whose raw azimuths span more than 180 degrees (max - min, pass 0; no scan
// throws 180 degrees) crosses 0 / 360: every az < 180 of it is used as az + 360.0 wherever the
// set-up reads az, so mu_k and sigma_k are those of the unwrapped series (mu_k may exceed 360) and
// its level is relative to azimuth on [180, 540).  Other groups keep the raw values.
//
// comap_destripe_ground_solve (end of this file) runs the whole CG on the device: the same
// launches per iteration on the problem's CG stream, gated by its device stop flag and replayed
// kCgBatch at a time as a captured graph, with the eager driver's arithmetic bit for bit.
//
// Layout: (group, pixel) entries twice, as the offset<->pixel operator is -- group-major for the
// projection (off-map reads kept with their negative pixel id, as opix) and pixel-major for the
// bin (binned entries only).  Both come from one stable radix sort of the samples by (group, read
// pixel, off-map) with segment sums in sample order, so the build is deterministic.  Group rows
// hold 1e4 .. 1e5 entries: they are cut into fixed chunks, one workgroup per chunk, and a finishing
// kernel adds each group's partials in chunk order.  No floating-point atomics anywhere.
#include "destriper_internal.h"

#include <rocprim/device/device_radix_sort.hpp>

struct comap_ground {
    comap_destriper *d = nullptr;
    comap_ctx *ctx = nullptr;
    int64_t NO = 0, npix = 0, K = 0;
    int64_t nnz = 0;            // group-major entries (incl. off-map reads)
    int64_t nnzb = 0;           // pixel-major entries (binned only)
    // offsets (internal order, d->perm)
    int32_t *gint = nullptr;    // [NO] group of internal offset i
    int32_t *glist = nullptr;   // [NO] internal offsets sorted by group (stable)
    double *wa = nullptr;       // [NO] sum w a
    // groups
    double *mu = nullptr, *sigma = nullptr, *saa = nullptr, *ta = nullptr;   // [K]
    // group-major entries
    int32_t *gpix = nullptr;    // [nnz] pixel (negative: an off-map read of m[npix + p])
    double *ga = nullptr;       // [nnz]
    // pixel-major entries
    int64_t *gprow = nullptr;   // [npix + 1]
    int32_t *gpk = nullptr;     // [nnzb] group
    double *gpa = nullptr;      // [nnzb]
    // reduction chunks: nce entry chunks then nco offset chunks, each (group, begin, end)
    int64_t nce = 0, nco = 0;
    int64_t *chunks = nullptr;  // [nce + nco][3]
    int64_t *cgrp = nullptr;    // [2 (K + 1)] each group's entry-chunk range, then its offset-chunk range
    double *part = nullptr;     // [nce + 2 nco] chunk partials
    int32_t *wrapped = nullptr; // [K] 1: the group crosses 0 / 360, its azimuths < 180 are used as az + 360
    // device-resident CG of comap_destripe_ground_solve (fixed pointers: graph-replayable); the
    // stream, scalars, stop flags and r.r partials are the plain problem's (d->cs, scal, flags, part)
    double *cg = nullptr;       // [4 (NO + 2K) + NO + npix + 1]: x, r, p, q | x' | num | the tails' r.r
    hipGraphExec_t batch = nullptr;   // kCgBatch iterations
    // scratch of the multi-rank pieces (comap_destripe_ground_dist_*), on their first use
    double *dist = nullptr;     // [NO + 1]: x' | the tails' r.r
};

namespace {

constexpr int64_t kChunkE = 1024;   // entries per projection workgroup (4 per thread: one pass of loads)
constexpr int64_t kChunkO = 1024;   // offsets per workgroup
constexpr int kBinLanes = 4;        // lanes per pixel row of the ground bin (rows hold <= K entries)

__device__ __forceinline__ int64_t wrap_pixel(int32_t p, int64_t npix) { return p >= 0 ? (int64_t)p : npix + p; }

__device__ __forceinline__ double map_value(const double *num, const double *h, int64_t q)
{
    const double hv = h[q];
    return hv != 0.0 ? num[q] / hv : num[q];
}

__device__ __forceinline__ int64_t lb32(const int32_t *a, int64_t n, int64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (a[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}

// fixed-order block sum (256 threads): wave sums, then the four waves' sums
__device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------- set-up
// gint[i] = gid[perm[i]] (flag[0]: an id outside [0, K)), val[i] = i
__global__ void k_gr_gint(const int32_t *__restrict__ gid, const int32_t *__restrict__ perm, int64_t NO, int64_t K,
                          int32_t *__restrict__ gint, int32_t *__restrict__ val, int32_t *__restrict__ flag)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < NO; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t g = gid[perm[i]];
        if (g < 0 || g >= K) { flag[0] = 1; g = 0; }
        gint[i] = g;
        val[i] = (int32_t)i;
    }
}

// row[k] = first sorted position with key >= k, k in [0, n_rows]
__global__ void k_gr_rowptr(const int32_t *__restrict__ skey, int64_t n, int64_t n_rows, int64_t *__restrict__ row)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k <= n_rows; k += (int64_t)gridDim.x * blockDim.x)
        row[k] = lb32(skey, n, k);
}

// The azimuth of a sample as the set-up uses it: a group that crosses 0 / 360 (wr) has its
// values below 180 moved up one turn -- one f64 add, before any arithmetic on the value.
__device__ __forceinline__ double unwrap_az(double v, bool wr) { return (wr && v < 180.0) ? v + 360.0 : v; }

// Per-offset sums over its L samples in sample order, a thread per internal offset i (offset
// perm[i]).  PASS 0: sum az, min, max.  PASS 1: sum (az - mu)^2.  PASS 2: sum w a, sum w a^2,
// sum w a tod with a = (az - mu) / sigma (0 when sigma == 0).  wrapped (NULL in the first pass 0,
// which finds the flags): the groups whose azimuths are unwrapped.
template <int PASS>
__global__ void __launch_bounds__(256) k_gr_offsets(const double *__restrict__ az, const double *__restrict__ w,
                                                    const double *__restrict__ tod, const int32_t *__restrict__ perm,
                                                    const int32_t *__restrict__ gint, const double *__restrict__ mu,
                                                    const double *__restrict__ sigma,
                                                    const int32_t *__restrict__ wrapped, int64_t NO, int L,
                                                    double *__restrict__ o0, double *__restrict__ o1,
                                                    double *__restrict__ o2)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < NO; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t0 = (int64_t)perm[i] * L;
        const int32_t k = gint[i];
        const bool wr = wrapped && wrapped[k];
        if constexpr (PASS == 0) {
            double s = 0.0, mn = unwrap_az(az[t0], wr), mx = mn;
            for (int j = 0; j < L; ++j) {
                const double v = unwrap_az(az[t0 + j], wr);
                s += v;
                mn = fmin(mn, v);
                mx = fmax(mx, v);
            }
            o0[i] = s; o1[i] = mn; o2[i] = mx;
        } else if constexpr (PASS == 1) {
            const double m = mu[k];
            double s = 0.0;
            for (int j = 0; j < L; ++j) {
                const double v = unwrap_az(az[t0 + j], wr) - m;
                s = fma(v, v, s);
            }
            o0[i] = s;
        } else {
            const double m = mu[k], sg = sigma[k];
            double sa = 0.0, saa = 0.0, sat = 0.0;
            for (int j = 0; j < L; ++j) {
                const double a = sg > 0.0 ? (unwrap_az(az[t0 + j], wr) - m) / sg : 0.0;
                const double wv = w[t0 + j] * a;
                sa += wv;
                saa = fma(wv, a, saa);
                sat = fma(wv, tod[t0 + j], sat);
            }
            o0[i] = sa; o1[i] = saa; o2[i] = sat;
        }
    }
}

// out[k] = sum (OP 0), min (1) or max (2) of v over group k's offsets, one workgroup per group,
// in a fixed order (thread-strided over the group's list, then the block)
template <int OP>
__global__ void __launch_bounds__(256) k_gr_group(const double *__restrict__ v, const int32_t *__restrict__ glist,
                                                  const int64_t *__restrict__ grow, double *__restrict__ out)
{
    __shared__ double red[4];
    const int64_t k = blockIdx.x, b = grow[k], e = grow[k + 1];
    double acc = OP == 0 ? 0.0 : (OP == 1 ? INFINITY : -INFINITY);
    for (int64_t j = b + threadIdx.x; j < e; j += 256) {
        const double x = v[glist[j]];
        acc = OP == 0 ? acc + x : (OP == 1 ? fmin(acc, x) : fmax(acc, x));
    }
    if constexpr (OP == 0) {
        acc = block_sum(acc, red);
    } else {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double y = __shfl_xor(acc, o, 64);
            acc = OP == 1 ? fmin(acc, y) : fmax(acc, y);
        }
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
        __syncthreads();
        acc = OP == 1 ? fmin(fmin(red[0], red[1]), fmin(red[2], red[3])) : fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    }
    if (threadIdx.x == 0) out[k] = acc;
}

// mu_k = sum az / n (0 for an empty group)
__global__ void k_gr_mean(const double *__restrict__ sum, const int64_t *__restrict__ grow, int64_t K, int L,
                          double *__restrict__ mu)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = (grow[k + 1] - grow[k]) * L;
        mu[k] = n ? sum[k] / (double)n : 0.0;
    }
}

// wrapped[k] = the group's raw azimuths span more than 180 degrees: it crosses 0 / 360 (no scan
// throws 180 degrees)
__global__ void k_gr_wrapflag(const double *__restrict__ mn, const double *__restrict__ mx,
                              const int64_t *__restrict__ grow, int64_t K, int32_t *__restrict__ wrapped)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x)
        wrapped[k] = (grow[k + 1] > grow[k] && mx[k] - mn[k] > 180.0) ? 1 : 0;
}

// sigma_k = sqrt(sum (az - mu)^2 / n); exactly 0 for an empty group or a constant azimuth
// (min == max: the rounded mean of equal values need not equal them)
__global__ void k_gr_rms(const double *__restrict__ sum, const double *__restrict__ mn, const double *__restrict__ mx,
                         const int64_t *__restrict__ grow, int64_t K, int L, double *__restrict__ sigma)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = (grow[k + 1] - grow[k]) * L;
        sigma[k] = (n && mx[k] > mn[k]) ? sqrt(sum[k] / (double)n) : 0.0;
    }
}

// Sort key of sample t: ((group, read pixel), off-map) -- the pixel the sample bins, or the
// one its projection reads through the wrap.  flag[0]: a group id outside [0, K); flag[1]: a
// pixel id outside [-npix, npix).
__global__ void k_gr_keys(const int32_t *__restrict__ pix, const int32_t *__restrict__ gid, int64_t N, int L,
                          int64_t npix, int64_t K, uint64_t *__restrict__ key, int32_t *__restrict__ flag)
{
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < N; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t k = gid[t / L];
        if (k < 0 || k >= K) { flag[0] = 1; k = 0; }
        int64_t p = pix[t];
        if (p >= npix || p < -npix) { flag[1] = 1; p = 0; }
        const int64_t q = p >= 0 ? p : npix + p;
        key[t] = (((uint64_t)k * (uint64_t)npix + (uint64_t)q) << 1) | (p < 0 ? 1u : 0u);
    }
}

// Entry e = the sorted samples [estart[e], estart[e + 1]): its group, pixel id (negative for an
// off-map read), ga_e = sum w a in sample order (the sort is stable), and its key for the
// pixel-major sort (the pixel; npix for an unbinned entry, which sorts behind every row).
__global__ void __launch_bounds__(256) k_gr_entries(const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                    const int32_t *__restrict__ estart, int64_t ne, int64_t N,
                                                    int64_t npix, const double *__restrict__ az,
                                                    const double *__restrict__ w, const double *__restrict__ mu,
                                                    const double *__restrict__ sigma,
                                                    const int32_t *__restrict__ wrapped, int32_t *__restrict__ egrp,
                                                    int32_t *__restrict__ gpix, double *__restrict__ ga,
                                                    int32_t *__restrict__ pkey, int32_t *__restrict__ pval)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = estart[e], i1 = e + 1 < ne ? (int64_t)estart[e + 1] : N;
        const uint64_t key = skey[i0];
        const bool off = key & 1u;
        const int64_t k = (int64_t)((key >> 1) / (uint64_t)npix), q = (int64_t)((key >> 1) % (uint64_t)npix);
        const double m = mu[k], sg = sigma[k];
        const bool wr = wrapped[k] != 0;
        double acc = 0.0;
        for (int64_t i = i0; i < i1; ++i) {
            const int64_t t = sval[i];
            const double a = sg > 0.0 ? (unwrap_az(az[t], wr) - m) / sg : 0.0;
            acc += w[t] * a;
        }
        egrp[e] = (int32_t)k;
        gpix[e] = (int32_t)(off ? q - npix : q);
        ga[e] = acc;
        pkey[e] = (int32_t)(off ? npix : q);
        pval[e] = (int32_t)e;
    }
}

// pixel-major copy of the binned entries (sorted position j < nnzb = row pointer of npix)
__global__ void k_gr_pixel_entries(const int32_t *__restrict__ spkey, const int32_t *__restrict__ spval, int64_t ne,
                                   int64_t npix, const int32_t *__restrict__ egrp, const double *__restrict__ ga,
                                   int32_t *__restrict__ gpk, double *__restrict__ gpa)
{
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < ne; j += (int64_t)gridDim.x * blockDim.x) {
        if (spkey[j] >= npix) continue;
        const int32_t e = spval[j];
        gpk[j] = egrp[e];
        gpa[j] = ga[e];
    }
}

// ---------------------------------------------------------------- per-iteration kernels
// The native solve's kernels return at once when the CG's device stop flag is set (flags[0],
// destriper_internal.h); the per-piece C ABI passes flags == NULL.
__device__ __forceinline__ bool gr_done(const int32_t *flags) { return flags && flags[0]; }

// x'_i = x_i + c_{g(i)}; wbar != NULL (the count form's bin input): also pt_i = wbar_i x'_i
__global__ void k_gr_fold(const double *__restrict__ x, const double *__restrict__ c, const int32_t *__restrict__ gint,
                          int64_t NO, double *__restrict__ xp, const double *__restrict__ wbar,
                          double *__restrict__ pt, const int32_t *__restrict__ flags)
{
    if (gr_done(flags)) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < NO; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = x[i] + c[gint[i]];
        xp[i] = v;
        if (wbar) pt[i] = wbar[i] * v;
    }
}

// num_p += sum_{e in pixel row p} ga_e (sign s_{k(e)}), sign = +-1: a gather per pixel row,
// kBinLanes lanes per row (lane-strided, then the lanes' sums); rows without entries are not written.
__global__ void __launch_bounds__(256) k_gr_bin(const int64_t *__restrict__ gprow, const int32_t *__restrict__ gpk,
                                                const double *__restrict__ gpa, const double *__restrict__ s,
                                                double sign, int64_t npix, double *__restrict__ num,
                                                const int32_t *__restrict__ flags)
{
    if (gr_done(flags)) return;
    const int sub = threadIdx.x & (kBinLanes - 1);
    const int64_t step = (int64_t)gridDim.x * blockDim.x / kBinLanes;
    for (int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kBinLanes; p < npix; p += step) {
        const int64_t e0 = gprow[p], e1 = gprow[p + 1];
        double acc = 0.0;
        for (int64_t j = e0 + sub; j < e1; j += kBinLanes) acc = fma(gpa[j], sign * s[gpk[j]], acc);
#pragma unroll
        for (int o = kBinLanes / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kBinLanes);
        if (sub == 0 && e1 > e0) num[p] += acc;
    }
}

// Chunk partials.  Workgroups [0, nce): sum of ga_e m[read pixel of e] over one chunk of a group
// row, m = num / h on the fly; each thread keeps 4 entry loads then 4 map gathers in flight.
// Workgroups [nce, nce + nco): one chunk of a group's offsets -- y_o += wa_o s_k (not for the
// right-hand side, s == NULL), partials of sum y_o and of sum wa_o x'_o.
__global__ void __launch_bounds__(256) k_gr_parts(const int64_t *__restrict__ chunks, int64_t nce,
                                                  const int32_t *__restrict__ gpix, const double *__restrict__ ga,
                                                  const double *__restrict__ num, const double *__restrict__ h,
                                                  int64_t npix, const int32_t *__restrict__ glist,
                                                  const double *__restrict__ wa, const double *__restrict__ xp,
                                                  const double *__restrict__ s, double *__restrict__ y,
                                                  double *__restrict__ part, const int32_t *__restrict__ flags)
{
    __shared__ double red[4];
    if (gr_done(flags)) return;
    const int64_t c = blockIdx.x;
    const int64_t k = chunks[3 * c], b = chunks[3 * c + 1], e = chunks[3 * c + 2];
    if (c < nce) {
        constexpr int U = 4;
        double acc = 0.0;
        for (int64_t j = b + threadIdx.x; j < e; j += 256 * U) {
            int64_t q[U];
            double a[U], m[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = j + u * 256 < e;
                q[u] = in ? wrap_pixel(gpix[j + u * 256], npix) : 0;
                a[u] = in ? ga[j + u * 256] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) m[u] = map_value(num, h, q[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (j + u * 256 < e) acc = fma(a[u], m[u], acc);
        }
        acc = block_sum(acc, red);
        if (threadIdx.x == 0) part[c] = acc;
    } else {
        const double sk = s ? s[k] : 0.0;
        double acc1 = 0.0, acca = 0.0;
        for (int64_t j = b + threadIdx.x; j < e; j += 256) {
            const int64_t o = glist[j];
            double yv = y[o];
            if (s) {
                const double wv = wa[o];
                yv = fma(wv, sk, yv);
                y[o] = yv;
                acca = fma(wv, xp[o], acca);
            }
            acc1 += yv;
        }
        acc1 = block_sum(acc1, red);
        acca = block_sum(acca, red);
        if (threadIdx.x == 0) {
            part[nce + 2 * (c - nce)] = acc1;
            part[nce + 2 * (c - nce) + 1] = acca;
        }
    }
}

// One wave per group: its chunk partials added in a fixed order (lane-strided in chunk order,
// then the wave).  z[k] = za_k (s == NULL: ba_k), z[K + k] = z1_k.
__global__ void __launch_bounds__(64) k_gr_finish(const int64_t *__restrict__ cgrp, int64_t K, int64_t nce,
                                                  const double *__restrict__ part, const double *__restrict__ saa,
                                                  const double *__restrict__ ta, const double *__restrict__ s,
                                                  double *__restrict__ z, const int32_t *__restrict__ flags)
{
    if (gr_done(flags)) return;
    const int64_t k = blockIdx.x;
    double ae = 0.0, a1 = 0.0, aa = 0.0;
    for (int64_t c = cgrp[k] + threadIdx.x; c < cgrp[k + 1]; c += 64) ae += part[c];
    for (int64_t c = cgrp[K + 1 + k] + threadIdx.x; c < cgrp[K + 2 + k]; c += 64) {
        a1 += part[nce + 2 * c];
        aa += part[nce + 2 * c + 1];
    }
    ae = wave_sum(ae);
    a1 = wave_sum(a1);
    aa = wave_sum(aa);
    if (threadIdx.x == 0) {
        z[k] = s ? (aa + saa[k] * s[k]) - ae : ta[k] - ae;
        z[K + k] = a1;
    }
}

// The CG's vector algebra on the 2K-value tails (s | c), one workgroup each; the offsets' part of
// every vector runs through the plain problem's kernels.  Sums are fixed-order.
// a . b over n tail values by one block: thread-strided fmas, then the block
__device__ __forceinline__ double tail_dot(const double *__restrict__ a, const double *__restrict__ b, int64_t n,
                                           double *red)
{
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) acc = fma(a[i], b[i], acc);
    return block_sum(acc, red);
}

// out += a . b
__global__ void __launch_bounds__(256) k_gr_tail_dot(const double *__restrict__ a, const double *__restrict__ b,
                                                     int64_t n, double *__restrict__ out)
{
    __shared__ double red[4];
    const double acc = tail_dot(a, b, n, red);
    if (threadIdx.x == 0) out[0] += acc;
}

// alpha = rr / pq; x += alpha p; r -= alpha q; rr_new += r . r (rr_new holds the offsets' part)
__global__ void __launch_bounds__(256) k_gr_tail_update(const double *__restrict__ rr, const double *__restrict__ pq,
                                                        double *__restrict__ x, double *__restrict__ r,
                                                        const double *__restrict__ p, const double *__restrict__ q,
                                                        int64_t n, double *__restrict__ rr_new)
{
    __shared__ double red[4];
    const double alpha = rr[0] / pq[0];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        x[i] += alpha * p[i];
        const double rv = r[i] - alpha * q[i];
        r[i] = rv;
        acc = fma(rv, rv, acc);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) rr_new[0] += acc;
}

// p = r + (rr_new / rr) p
__global__ void __launch_bounds__(256) k_gr_tail_direction(const double *__restrict__ rr_new,
                                                           const double *__restrict__ rr, double *__restrict__ p,
                                                           const double *__restrict__ r, int64_t n)
{
    const double beta = rr_new[0] / rr[0];
    for (int64_t i = threadIdx.x; i < n; i += 256) p[i] = r[i] + beta * p[i];
}

// The native solve's update and direction over whole vectors [x | s | c]: the arithmetic and the
// summation orders of the eager driver's calls -- comap_destripe_dot / _cg_update / _cg_direction
// on the NO offsets, then the one-workgroup tail kernels above on the 2K tail values -- so the
// iterates equal the eager driver's bit for bit (the operator has a null space, and CG on it
// magnifies a rounding difference by many orders of magnitude within some iterations), folded
// into two gated launches.  Every block re-derives the sums from the partials in the same fixed
// order, so all hold identical values; block 0 also advances the tails.
//   k_gr_update: p.q = sum(part_pq, k_dot_part's partials of the offsets) + the tails' p.q;
//       a = rr / p.q; x += a p; r -= a q; r.r partials of the offsets into part_rr (k_cg_update's
//       grid), the tails' r.r into tail_rr; block 0 saves rr and p.q
// SPLIT (the multi-rank pieces, cut at the all-reduces): p.q is read from scal[2], where
// k_gr_pq left the rank's sum for the caller to all-reduce, and k_gr_rr takes the r.r final.
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_gr_update(double *__restrict__ scal, const double *__restrict__ part_pq,
                                                   double *__restrict__ x, double *__restrict__ r,
                                                   const double *__restrict__ p, const double *__restrict__ q,
                                                   int64_t NO, int64_t K, double *__restrict__ part_rr,
                                                   double *__restrict__ tail_rr, const int32_t *__restrict__ flags)
{
    __shared__ double red[4];
    if (gr_done(flags)) return;
    double pq;
    if constexpr (SPLIT) {
        pq = scal[2];
    } else {
        pq = block_final_sum(part_pq, kRedBlocks, red);
        pq += tail_dot(p + NO, q + NO, 2 * K, red);
    }
    const double rr = scal[3];
    const double a[1] = {rr / pq};
    const bool live[1] = {true};
    double acc[1] = {0.0};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < NO; i += (int64_t)gridDim.x * blockDim.x)
        update_row<1>(x + i, r + i, p + i, q + i, a, live, acc);
    const double bs = block_sum(acc[0], red);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = bs;
    if (blockIdx.x == 0) {
        const double alpha = a[0];
        double t = 0.0;
        for (int64_t i = NO + threadIdx.x; i < NO + 2 * K; i += 256) {
            x[i] += alpha * p[i];
            const double rv = r[i] - alpha * q[i];
            r[i] = rv;
            t = fma(rv, rv, t);
        }
        t = block_sum(t, red);
        if (threadIdx.x == 0) {
            tail_rr[0] = t;
            scal[1] = rr;
            if constexpr (!SPLIT) scal[2] = pq;
        }
    }
}

//   k_gr_direction: rr_new = sum(part_rr) + tail_rr; p = r + (rr_new / rr) p; block 0, after its
//       own sweep: rr = rr_new, count the iteration, stop when rr_new / rr0 is NaN or below the
//       threshold (scal / flags: the one-band layout of destriper_internal.h)
// SPLIT: rr_new is read from scal[3], the all-reduced sum of k_gr_rr's.
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_gr_direction(double *__restrict__ scal, const double *__restrict__ part_rr,
                                                      int nrr, const double *__restrict__ tail_rr,
                                                      double *__restrict__ p, const double *__restrict__ r, int64_t NO,
                                                      int64_t K, int32_t *flags)
{
    __shared__ double red[4];
    if (flags[0]) return;
    double rrn;
    if constexpr (SPLIT) {
        rrn = scal[3];
    } else {
        rrn = block_final_sum(part_rr, nrr, red);
        rrn += tail_rr[0];
    }
    const double beta[1] = {rrn / scal[1]};
    const bool live[1] = {true};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < NO; i += (int64_t)gridDim.x * blockDim.x)
        direction_row<1>(p + i, r + i, beta, live);
    if (blockIdx.x == 0) {
        for (int64_t i = NO + threadIdx.x; i < NO + 2 * K; i += 256) p[i] = r[i] + beta[0] * p[i];
        if (threadIdx.x == 0) {
            if constexpr (!SPLIT) scal[3] = rrn;   // (split: other blocks may still be reading it)
            flags[3] += 1;
            flags[1] += 1;
            const double delta = rrn / scal[0];
            if (isnan(delta) || delta < scal[4]) { flags[2] = 1; flags[0] = 1; }
        }
    }
}

// The multi-rank pieces' two scalar finals, one workgroup each, in the order of the eager calls
// (k_dot_final's sum of the offsets' partials, then the tails' part added):
//   k_gr_pq: scal[2] = sum(part, comap_destripe_dot's grid) + the tails' p . q
__global__ void __launch_bounds__(256) k_gr_pq(const double *__restrict__ part, const double *__restrict__ p,
                                               const double *__restrict__ q, int64_t NO, int64_t K,
                                               double *__restrict__ scal, const int32_t *__restrict__ flags)
{
    __shared__ double red[4];
    if (gr_done(flags)) return;
    double pq = block_final_sum(part, kRedBlocks, red);
    pq += tail_dot(p + NO, q + NO, 2 * K, red);
    if (threadIdx.x == 0) scal[2] = pq;
}

//   k_gr_rr: scal[3] = sum(part_rr, comap_destripe_cg_update's grid) + the tails' r . r
__global__ void __launch_bounds__(256) k_gr_rr(const double *__restrict__ part_rr, int nrr,
                                               const double *__restrict__ tail_rr, double *__restrict__ scal,
                                               const int32_t *__restrict__ flags)
{
    __shared__ double red[4];
    if (gr_done(flags)) return;
    double rrn = block_final_sum(part_rr, nrr, red);
    rrn += tail_rr[0];
    if (threadIdx.x == 0) scal[3] = rrn;
}

void ground_free(comap_ground *g, bool idle)
{
    if (g->batch) (void)hipGraphExecDestroy(g->batch);
    void *b[] = {g->gint, g->glist, g->wa, g->mu, g->sigma, g->saa, g->ta, g->gpix, g->ga, g->gprow, g->gpk, g->gpa,
                 g->chunks, g->cgrp, g->part, g->wrapped, g->cg, g->dist};
    comap_tmp_free_on(b, (int)(sizeof(b) / sizeof(b[0])), nullptr, idle);
    delete g;
}

int ground_build(comap_ground *g, const int32_t *pix, const double *az, const double *tod, const double *w,
                 const int32_t *gid)
{
    comap_destriper *d = g->d;
    comap_ctx *ctx = g->ctx;
    hipStream_t st = ctx->stream;
    const int64_t N = d->N, NO = d->NO, npix = d->npix, K = g->K;
    const int L = d->L;
    int rc = 0;
    rc |= dalloc(ctx, &g->gint, NO);
    rc |= dalloc(ctx, &g->glist, NO);
    rc |= dalloc(ctx, &g->wa, NO);
    rc |= dalloc(ctx, &g->mu, K);
    rc |= dalloc(ctx, &g->sigma, K);
    rc |= dalloc(ctx, &g->saa, K);
    rc |= dalloc(ctx, &g->ta, K);
    rc |= dalloc(ctx, &g->wrapped, K);
    rc |= dalloc(ctx, &g->gprow, npix + 1);
    rc |= dalloc(ctx, &g->cgrp, 2 * (K + 1));
    if (rc) return -2;

    DevTemps tmp(st);
    const int64_t nmax = std::max<int64_t>(N, std::max<int64_t>(NO, K + 1));
    uint64_t *key = nullptr;
    int32_t *val = nullptr, *gs = nullptr, *flag = nullptr;
    double *ov = nullptr, *gv = nullptr;
    int64_t *grow = nullptr, *garow = nullptr;
    COMAP_CHECK(ctx, tmp.alloc(&key, N));
    COMAP_CHECK(ctx, tmp.alloc(&val, nmax));
    COMAP_CHECK(ctx, tmp.alloc(&gs, NO));
    COMAP_CHECK(ctx, tmp.alloc(&flag, 2));
    COMAP_CHECK(ctx, tmp.alloc(&ov, 3 * NO));
    COMAP_CHECK(ctx, tmp.alloc(&gv, 3 * K));
    COMAP_CHECK(ctx, tmp.alloc(&grow, K + 1));
    COMAP_CHECK(ctx, tmp.alloc(&garow, K + 1));
    const int kbits = bits_for((uint64_t)K), pbits = bits_for((uint64_t)npix + 1);
    const int sbits = bits_for((uint64_t)K * (uint64_t)npix * 2u);
    // sort scratch of steps 1 and 4 (the latter's size is bounded by N); step 3's is the helper's own
    size_t tb = 0, b1 = 0;
    COMAP_CHECK(ctx, rocprim::radix_sort_pairs(nullptr, b1, val, gs, val, gs, (size_t)NO, 0u, (unsigned)kbits, st));
    tb = std::max(tb, b1);
    COMAP_CHECK(ctx, rocprim::radix_sort_pairs(nullptr, b1, val, val, val, val, (size_t)N, 0u, (unsigned)pbits, st));
    tb = std::max(tb, b1);
    char *cub = nullptr;
    COMAP_CHECK(ctx, tmp.alloc(&cub, tb));

    // ---- 1. the offsets' groups in the internal order, and each group's offset list
    COMAP_CHECK(ctx, hipMemsetAsync(flag, 0, 8, st));
    k_gr_gint<<<grid_for(NO), 256, 0, st>>>(gid, d->perm, NO, K, g->gint, val, flag);
    COMAP_LAUNCH_CHECK(ctx);
    b1 = tb;
    COMAP_CHECK(ctx, rocprim::radix_sort_pairs(cub, b1, g->gint, gs, val, g->glist, (size_t)NO, 0u, (unsigned)kbits, st));
    k_gr_rowptr<<<grid_for(K + 1), 256, 0, st>>>(gs, NO, K, grow);
    COMAP_LAUNCH_CHECK(ctx);

    // ---- 2. mu, sigma per group; wa per offset; Saa, Ta per group
    // (pass 0 twice: on the raw azimuths for each group's span, hence its wrap flag, then on the
    // unwrapped values -- for a group that is not flagged the same arithmetic on the same values)
    double *o0 = ov, *o1 = ov + NO, *o2 = ov + 2 * NO;
    k_gr_offsets<0><<<grid_for(NO), 256, 0, st>>>(az, w, tod, d->perm, g->gint, nullptr, nullptr, nullptr, NO, L, o0,
                                                  o1, o2);
    k_gr_group<1><<<(unsigned)K, 256, 0, st>>>(o1, g->glist, grow, gv + K);
    k_gr_group<2><<<(unsigned)K, 256, 0, st>>>(o2, g->glist, grow, gv + 2 * K);
    k_gr_wrapflag<<<grid_for(K), 256, 0, st>>>(gv + K, gv + 2 * K, grow, K, g->wrapped);
    k_gr_offsets<0><<<grid_for(NO), 256, 0, st>>>(az, w, tod, d->perm, g->gint, nullptr, nullptr, g->wrapped, NO, L,
                                                  o0, o1, o2);
    k_gr_group<0><<<(unsigned)K, 256, 0, st>>>(o0, g->glist, grow, gv);
    k_gr_group<1><<<(unsigned)K, 256, 0, st>>>(o1, g->glist, grow, gv + K);
    k_gr_group<2><<<(unsigned)K, 256, 0, st>>>(o2, g->glist, grow, gv + 2 * K);
    k_gr_mean<<<grid_for(K), 256, 0, st>>>(gv, grow, K, L, g->mu);
    k_gr_offsets<1><<<grid_for(NO), 256, 0, st>>>(az, w, tod, d->perm, g->gint, g->mu, nullptr, g->wrapped, NO, L, o0,
                                                  o1, o2);
    k_gr_group<0><<<(unsigned)K, 256, 0, st>>>(o0, g->glist, grow, gv);
    k_gr_rms<<<grid_for(K), 256, 0, st>>>(gv, gv + K, gv + 2 * K, grow, K, L, g->sigma);
    k_gr_offsets<2><<<grid_for(NO), 256, 0, st>>>(az, w, tod, d->perm, g->gint, g->mu, g->sigma, g->wrapped, NO, L,
                                                  g->wa, o1, o2);
    k_gr_group<0><<<(unsigned)K, 256, 0, st>>>(o1, g->glist, grow, g->saa);
    k_gr_group<0><<<(unsigned)K, 256, 0, st>>>(o2, g->glist, grow, g->ta);
    COMAP_LAUNCH_CHECK(ctx);

    // ---- 3. the samples sorted by (group, read pixel, off-map); one entry per distinct key
    // (ds_sorted_segments, destriper_segments.hip: read-back 1 -- entries, flags)
    k_gr_keys<<<grid_for(N, 65536), 256, 0, st>>>(pix, gid, N, L, npix, K, key, flag);
    COMAP_LAUNCH_CHECK(ctx);
    ds_segments<uint64_t> seg;
    if (const int src = ds_sorted_segments(ctx, tmp, key, N, sbits, flag, &seg)) return src;
    if (seg.flag[0]) return comap_fail(ctx, -3, "ground group id out of range (valid: 0 .. n_groups - 1)");
    if (seg.flag[1]) return comap_fail(ctx, -3, "pixel index out of range for the map (>= npix or < -npix)");
    const int64_t ne = seg.ne;
    if (ne < 1 || ne > N) return comap_fail(ctx, -2, "ground set-up: bad entry count");
    g->nnz = ne;

    // ---- 4. the group-major entries, then their pixel-major copy
    int32_t *egrp = nullptr, *pkey = nullptr, *spkey = nullptr;
    rc |= dalloc(ctx, &g->gpix, ne);
    rc |= dalloc(ctx, &g->ga, ne);
    rc |= dalloc(ctx, &g->gpk, ne);        // nnzb <= nnz
    rc |= dalloc(ctx, &g->gpa, ne);
    if (rc) return -2;
    COMAP_CHECK(ctx, tmp.alloc(&egrp, ne));
    COMAP_CHECK(ctx, tmp.alloc(&pkey, ne));
    COMAP_CHECK(ctx, tmp.alloc(&spkey, ne));
    // (val is free again: the pixel-major sort's values)
    k_gr_entries<<<grid_for(ne, 65536), 256, 0, st>>>(seg.skey, seg.sval, seg.estart, ne, N, npix, az, w, g->mu, g->sigma,
                                                      g->wrapped, egrp, g->gpix, g->ga, pkey, val);
    k_gr_rowptr<<<grid_for(K + 1), 256, 0, st>>>(egrp, ne, K, garow);
    COMAP_LAUNCH_CHECK(ctx);
    int32_t *spval = seg.estart;           // (the segment starts are consumed)
    COMAP_CHECK(ctx, rocprim::radix_sort_pairs(nullptr, b1, pkey, spkey, val, spval, (size_t)ne, 0u, (unsigned)pbits, st));
    if (b1 > tb) {
        tb = b1;
        COMAP_CHECK(ctx, tmp.alloc(&cub, tb));
    }
    b1 = tb;
    COMAP_CHECK(ctx, rocprim::radix_sort_pairs(cub, b1, pkey, spkey, val, spval, (size_t)ne, 0u, (unsigned)pbits, st));
    k_gr_rowptr<<<grid_for(npix + 1), 256, 0, st>>>(spkey, ne, npix, g->gprow);
    k_gr_pixel_entries<<<grid_for(ne, 65536), 256, 0, st>>>(spkey, spval, ne, npix, egrp, g->ga, g->gpk, g->gpa);
    COMAP_LAUNCH_CHECK(ctx);

    // ---- 5. read-back 2: the groups' row bounds; the reduction chunks
    std::vector<int64_t> hrow(2 * (K + 1) + 1);
    COMAP_CHECK(ctx, hipMemcpyAsync(hrow.data(), garow, 8 * (size_t)(K + 1), hipMemcpyDeviceToHost, st));
    COMAP_CHECK(ctx, hipMemcpyAsync(hrow.data() + K + 1, grow, 8 * (size_t)(K + 1), hipMemcpyDeviceToHost, st));
    COMAP_CHECK(ctx, hipMemcpyAsync(hrow.data() + 2 * (K + 1), g->gprow + npix, 8, hipMemcpyDeviceToHost, st));
    COMAP_CHECK(ctx, hipStreamSynchronize(st));
    g->nnzb = hrow[2 * (K + 1)];
    if (hrow[K] != ne || hrow[2 * K + 1] != NO || g->nnzb < 0 || g->nnzb > ne)
        return comap_fail(ctx, -2, "ground set-up: inconsistent row bounds");
    std::vector<int64_t> ch, cg(2 * (K + 1));
    for (int pass = 0; pass < 2; ++pass) {
        const int64_t *row = hrow.data() + pass * (K + 1);
        const int64_t step = pass ? kChunkO : kChunkE;
        int64_t n = 0;
        for (int64_t k = 0; k < K; ++k) {
            cg[pass * (K + 1) + k] = n;
            for (int64_t b = row[k]; b < row[k + 1]; b += step, ++n) {
                ch.push_back(k);
                ch.push_back(b);
                ch.push_back(std::min(b + step, row[k + 1]));
            }
        }
        cg[pass * (K + 1) + K] = n;
        (pass ? g->nco : g->nce) = n;
    }
    const int64_t nc = g->nce + g->nco;
    rc |= dalloc(ctx, &g->chunks, 3 * nc);
    rc |= dalloc(ctx, &g->part, g->nce + 2 * g->nco);
    if (rc) return -2;
    COMAP_CHECK(ctx, comap_upload(g->chunks, ch.data(), 8 * ch.size(), st));
    COMAP_CHECK(ctx, comap_upload(g->cgrp, cg.data(), 8 * cg.size(), st));
    return 0;
}

}  // namespace

extern "C" int comap_destripe_ground_create(comap_destriper *d, const int32_t *pix, const double *az, const double *tod,
                                            const double *w, const int32_t *gid, int64_t n_groups, comap_ground **out)
{
    if (!d || !out) return -1;
    comap_ctx *ctx = d->ctx;
    if (!pix || !az || !tod || !w || !gid) return comap_fail(ctx, -1, "ground template: null input");
    if (d->nb != 1) return comap_fail(ctx, -1, "ground template: one band per problem (batched bands are not supported)");
    if (n_groups < 1 || n_groups > (1 << 24)) return comap_fail(ctx, -1, "ground template: 1 .. 2^24 groups");
    if (d->N >= (int64_t(1) << 31) || d->npix >= (int64_t(1) << 31) - 1)
        return comap_fail(ctx, -1, "ground template: sample and pixel counts must fit 31 bits");
    if ((uint64_t)n_groups * (uint64_t)d->npix >= (uint64_t(1) << 62))
        return comap_fail(ctx, -1, "ground template: groups x pixels must fit 62 bits");
    COMAP_DEVICE_GUARD(ctx);
    comap_ground *g = new comap_ground;
    g->d = d;
    g->ctx = ctx;
    g->NO = d->NO;
    g->npix = d->npix;
    g->K = n_groups;
    const int rc = ground_build(g, pix, az, tod, w, gid);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        ground_free(g, true);
        return rc;
    }
    *out = g;
    return 0;
}

extern "C" int comap_destripe_ground_destroy(comap_ground *g)
{
    if (!g) return 0;
    COMAP_DEVICE_GUARD(g->ctx);
    (void)hipDeviceSynchronize();
    ground_free(g, true);
    return 0;
}

extern "C" int64_t comap_destripe_ground_n_groups(const comap_ground *g) { return g ? g->K : -1; }

extern "C" int comap_destripe_ground_nnz(const comap_ground *g, int64_t *nnz_group_major, int64_t *nnz_pixel_major)
{
    if (!g) return -1;
    if (nnz_group_major) *nnz_group_major = g->nnz;
    if (nnz_pixel_major) *nnz_pixel_major = g->nnzb;
    return 0;
}

extern "C" int comap_destripe_ground_stats(comap_ground *g, double *mu, double *sigma)
{
    if (!g) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    const size_t b = 8 * (size_t)g->K;
    if (mu) COMAP_CHECK(ctx, hipMemcpyAsync(mu, g->mu, b, hipMemcpyDeviceToDevice, ctx->stream));
    if (sigma) COMAP_CHECK(ctx, hipMemcpyAsync(sigma, g->sigma, b, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

extern "C" int comap_destripe_ground_fold(comap_ground *g, const double *x, const double *c, double *xprime)
{
    if (!g || !x || !c || !xprime) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    k_gr_fold<<<grid_for(g->NO), 256, 0, ctx->stream>>>(x, c, g->gint, g->NO, xprime, nullptr, nullptr, nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_ground_wrapped(comap_ground *g, int32_t *flag)
{
    if (!g || !flag) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    COMAP_CHECK(ctx, hipMemcpyAsync(flag, g->wrapped, 4 * (size_t)g->K, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

extern "C" int comap_destripe_ground_bin(comap_ground *g, const double *s, double *num)
{
    if (!g || !s || !num) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    k_gr_bin<<<grid_for(g->npix * kBinLanes, 65536), 256, 0, ctx->stream>>>(g->gprow, g->gpk, g->gpa, s, 1.0, g->npix,
                                                                            num, nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

// The ground projection on stream st (flags: the native solve's stop flags, or NULL)
static void launch_ground_project(comap_ground *g, hipStream_t st, const double *xprime, const double *s,
                                  const double *num, const double *h, double *y, double *z, const int32_t *flags)
{
    const int64_t nc = g->nce + g->nco;
    if (nc)
        k_gr_parts<<<(unsigned)nc, 256, 0, st>>>(g->chunks, g->nce, g->gpix, g->ga, num, h, g->npix, g->glist, g->wa,
                                                 xprime, s, y, g->part, flags);
    k_gr_finish<<<(unsigned)g->K, 64, 0, st>>>(g->cgrp, g->K, g->nce, g->part, g->saa, g->ta, s, z, flags);
}

static int ground_project(comap_ground *g, const double *xprime, const double *s, const double *num, const double *h,
                          double *y, double *z)
{
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    launch_ground_project(g, ctx->stream, xprime, s, num, h ? h : g->d->h, y, z, nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_ground_project(comap_ground *g, const double *xprime, const double *s, const double *num,
                                             const double *h, double *y, double *z)
{
    if (!g || !xprime || !s || !num || !y || !z) return -1;
    return ground_project(g, xprime, s, num, h, y, z);
}

extern "C" int comap_destripe_ground_rhs(comap_ground *g, const double *num, const double *h, const double *b, double *z)
{
    if (!g || !num || !b || !z) return -1;
    // (the right-hand side reads b and leaves it as it is)
    return ground_project(g, nullptr, nullptr, num, h, const_cast<double *>(b), z);
}

extern "C" int comap_destripe_ground_tail_dot(comap_ground *g, const double *a, const double *b, double *dot)
{
    if (!g || !a || !b || !dot) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    k_gr_tail_dot<<<1, 256, 0, ctx->stream>>>(a, b, 2 * g->K, dot);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_ground_tail_update(comap_ground *g, const double *rr, const double *pq, double *x,
                                                 double *r, const double *p, const double *q, double *rr_new)
{
    if (!g || !rr || !pq || !x || !r || !p || !q || !rr_new) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    k_gr_tail_update<<<1, 256, 0, ctx->stream>>>(rr, pq, x, r, p, q, 2 * g->K, rr_new);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_ground_tail_direction(comap_ground *g, const double *rr_new, const double *rr, double *p,
                                                    const double *r)
{
    if (!g || !rr_new || !rr || !p || !r) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    k_gr_tail_direction<<<1, 256, 0, ctx->stream>>>(rr_new, rr, p, r, 2 * g->K);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

// The matvec q = A p of the native iteration and of the multi-rank pieces, cut where the map
// numerator is summed across ranks.  First half: x' = p + c[g(o)] (count form: and the bin's
// input pt = wbar o x'), num = W x' (undivided), then the ground bin.
static void launch_fold_bin(comap_ground *g, hipStream_t st, const double *p, double *xp, double *num,
                            const int32_t *flags)
{
    comap_destriper *d = g->d;
    const int64_t NO = g->NO;
    k_gr_fold<<<grid_for(NO), 256, 0, st>>>(p, p + NO + g->K, g->gint, NO, xp, d->cf ? d->wbar : nullptr, d->pt, flags);
    // (every row, as comap_destripe_bin: the hit-row bin sizes its lanes differently, another summation order)
    ds_launch_bin(d, st, d->cf ? d->pt : xp, nullptr, nullptr, num, flags, false, d->cf);
    k_gr_bin<<<grid_for(g->npix * kBinLanes, 65536), 256, 0, st>>>(g->gprow, g->gpk, g->gpa, p + NO, 1.0, g->npix, num,
                                                                   flags);
}

// second half: q = the projection (m = num / h on the fly), the ground projection, then the
// offsets' p.q partials on the finished q (d->part)
static void launch_project_dot(comap_ground *g, hipStream_t st, const double *p, const double *xp, const double *num,
                               const double *h, double *q, const int32_t *flags)
{
    const int64_t NO = g->NO;
    ds_launch_project(g->d, st, xp, num, h, q, flags);
    launch_ground_project(g, st, xp, p + NO, num, h, q, q + NO, flags);
    ds_dot_part(g->d, st, p, q, NO);   // not gated: it writes the partials only
}

// ---------------------------------------------------------------- device-resident ground CG
// One CG iteration on the ground object's own vectors u = [x | s | c] (n = NO + 2K values each):
// the launches of the eager driver's matvec with their arguments (launch_fold_bin,
// launch_project_dot), and its dot finals, update, tail update, direction, tail direction and
// stop test folded into k_gr_update / k_gr_direction.
// 9 launches (the count form's scaling rides in the fold), all but the partials' gated by the
// stop flag; the iterates are the eager driver's bit for bit.
static void ground_enqueue_iteration(comap_ground *g, hipStream_t st)
{
    comap_destriper *d = g->d;
    const int64_t NO = g->NO, K = g->K, n = NO + 2 * K;
    double *x = g->cg, *r = x + n, *p = r + n, *q = p + n, *xp = q + n, *num = xp + NO, *tail_rr = num + g->npix;
    int32_t *flags = d->flags;
    double *part_rr = d->part + kPartMax;
    launch_fold_bin(g, st, p, xp, num, flags);
    launch_project_dot(g, st, p, xp, num, d->h, q, flags);
    const unsigned ug = ds_upd_grid(NO);
    k_gr_update<false><<<ug, 256, 0, st>>>(d->scal, d->part, x, r, p, q, NO, K, part_rr, tail_rr, flags);
    k_gr_direction<false><<<grid_for(NO), 256, 0, st>>>(d->scal, part_rr, (int)ug, tail_rr, p, r, NO, K, flags);
}

// CG vectors and (small problems, or COMAP_DS_CGGRAPH=1) the kCgBatch-iteration graph, on first use
static int ground_cg_setup(comap_ground *g)
{
    comap_destriper *d = g->d;
    comap_ctx *ctx = g->ctx;
    if (g->cg && (g->batch || !ds_cg_use_graph(d))) return 0;
    const int64_t n = g->NO + 2 * g->K;
    if (!g->cg && dalloc(ctx, &g->cg, 4 * (size_t)n + (size_t)g->NO + (size_t)g->npix + 1)) return -2;
    if (const int rc = ds_cg_state(d)) return rc;
    if (!ds_cg_use_graph(d)) return 0;
    // (the vectors were allocated in the context stream's order: the capture below only records)
    hipGraph_t gr = nullptr;
    COMAP_CHECK(ctx, hipStreamBeginCapture(d->cs, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < kCgBatch; ++i) ground_enqueue_iteration(g, d->cs);
    COMAP_CHECK(ctx, hipStreamEndCapture(d->cs, &gr));
    const hipError_t e = hipGraphInstantiate(&g->batch, gr, nullptr, nullptr, 0);
    (void)hipGraphDestroy(gr);
    COMAP_CHECK(ctx, e);
    return 0;
}

// cg_solve(GroundOps, identity, threshold, niter) without Python per iteration: kCgBatch iterations
// per graph launch and host check, a remainder below kCgBatch as plain launches; the device stop
// flag makes the iterations queued behind convergence no-ops.  Then the maps, as _solve_ground.
extern "C" int comap_destripe_ground_solve(comap_ground *g, double threshold, int32_t niter, double *u, double *map,
                                           double *naive, double *weight, double *hits, int32_t *iters_out)
{
    if (!g || !u || niter < 0) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    comap_destriper *d = g->d;
    int rc = ground_cg_setup(g);
    if (rc) return rc;
    hipStream_t st = d->cs;
    const int64_t NO = g->NO, K = g->K, n = NO + 2 * K, np = g->npix;
    double *x = g->cg, *r = x + n, *p = r + n, *xp = p + 2 * n, *num = xp + NO;
    // inputs (and the vectors' allocation) are ordered on the caller's stream
    COMAP_CHECK(ctx, hipEventRecord(d->ev, ctx->stream));
    COMAP_CHECK(ctx, hipStreamWaitEvent(st, d->ev, 0));
    d->thr_host[0] = threshold;
    COMAP_CHECK(ctx, hipMemcpyAsync(d->scal + 4, d->thr_host, 8, hipMemcpyHostToDevice, st));
    COMAP_CHECK(ctx, hipMemsetAsync(x, 0, 8 * (size_t)n, st));
    COMAP_CHECK(ctx, hipMemsetAsync(d->flags, 0, 4 * 4, st));
    // b: the offsets' rows, then the tail from them; r = p = b (u0 = 0); rr = rr0 = b.b
    ds_launch_project(d, st, nullptr, d->nnum, d->h, r, nullptr);
    launch_ground_project(g, st, nullptr, nullptr, d->nnum, d->h, r, r + NO, nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    COMAP_CHECK(ctx, hipMemcpyAsync(p, r, 8 * (size_t)n, hipMemcpyDeviceToDevice, st));
    ds_dot(d, st, r, r, NO, d->scal);
    k_gr_tail_dot<<<1, 256, 0, st>>>(r + NO, r + NO, 2 * K, d->scal);
    COMAP_LAUNCH_CHECK(ctx);
    COMAP_CHECK(ctx, hipMemcpyAsync(d->scal + 1, d->scal, 8, hipMemcpyDeviceToDevice, st));
    COMAP_CHECK(ctx, hipMemcpyAsync(d->scal + 3, d->scal, 8, hipMemcpyDeviceToDevice, st));   // current rr
    for (int i = 0; i < 4; ++i) d->flags_host[i] = 0;
    for (int enq = 0; enq < niter;) {
        const int k = std::min(kCgBatch, niter - enq);
        if (k == kCgBatch && g->batch) {
            COMAP_CHECK(ctx, hipGraphLaunch(g->batch, st));
        } else {
            for (int i = 0; i < k; ++i) ground_enqueue_iteration(g, st);
            COMAP_LAUNCH_CHECK(ctx);
        }
        enq += k;
        COMAP_CHECK(ctx, hipMemcpyAsync(d->flags_host, d->flags, 4 * 4, hipMemcpyDeviceToHost, st));
        COMAP_CHECK(ctx, hipStreamSynchronize(st));
        if (d->flags_host[0]) break;
    }
    if (iters_out) iters_out[0] = d->flags_host[3];
    COMAP_CHECK(ctx, hipMemcpyAsync(u, x, 8 * (size_t)n, hipMemcpyDeviceToDevice, st));
    // final maps: map = (sum w tod - W x' - ground bin(s)) / h ; naive = sum w tod / h
    if (map) {
        k_gr_fold<<<grid_for(NO), 256, 0, st>>>(x, x + NO + K, g->gint, NO, xp, nullptr, nullptr, nullptr);
        ds_launch_bin(d, st, xp, d->nnum, nullptr, num, nullptr, false, false);
        k_gr_bin<<<grid_for(np * kBinLanes, 65536), 256, 0, st>>>(g->gprow, g->gpk, g->gpa, x + NO, -1.0, np, num,
                                                                  nullptr);
        ds_div_map(st, num, d->h, np, map);
    }
    if (naive) ds_div_map(st, d->nnum, d->h, np, naive);
    COMAP_LAUNCH_CHECK(ctx);
    if (weight) COMAP_CHECK(ctx, hipMemcpyAsync(weight, d->h, 8 * (size_t)np, hipMemcpyDeviceToDevice, st));
    if (hits) COMAP_CHECK(ctx, hipMemcpyAsync(hits, d->hits, 8 * (size_t)np, hipMemcpyDeviceToDevice, st));
    COMAP_CHECK(ctx, hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------- multi-rank CG pieces
// ground_enqueue_iteration cut at its three cross-rank sums (map numerator, p.q, r.r), on the
// caller's vectors [x | s | c] and scalars, on the bound stream.  The launches and their arguments are
// the native iteration's; only the two scalar finals, which there ride in k_gr_update /
// k_gr_direction, are kernels of their own (k_gr_pq, k_gr_rr), because an all-reduce follows each.
// Every local sum keeps the order of the eager per-piece calls, so the iterates equal those of
// Python's cg_solve on the same ranks bit for bit.
static int ground_dist_scratch(comap_ground *g)
{
    if (g->dist) return 0;
    return dalloc(g->ctx, &g->dist, (size_t)g->NO + 1) ? -2 : 0;
}

extern "C" int comap_destripe_ground_dist_bin(comap_ground *g, const double *p, double *num, const int32_t *flags)
{
    if (!g || !p || !num || !flags) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    if (const int rc = ground_dist_scratch(g)) return rc;
    launch_fold_bin(g, ctx->stream, p, g->dist, num, flags);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_ground_dist_project(comap_ground *g, const double *p, const double *num, const double *h,
                                                  double *q, double *scal, const int32_t *flags)
{
    if (!g || !p || !num || !h || !q || !scal || !flags) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    if (!g->dist) return comap_fail(ctx, -1, "ground dist_project: call comap_destripe_ground_dist_bin on p first");
    launch_project_dot(g, ctx->stream, p, g->dist, num, h, q, flags);
    k_gr_pq<<<1, 256, 0, ctx->stream>>>(g->d->part, p, q, g->NO, g->K, scal, flags);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_ground_dist_update(comap_ground *g, double *scal, double *x, double *r, const double *p,
                                                 const double *q, const int32_t *flags)
{
    if (!g || !scal || !x || !r || !p || !q || !flags) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    comap_destriper *d = g->d;
    if (const int rc = ground_dist_scratch(g)) return rc;
    hipStream_t st = ctx->stream;
    const int64_t NO = g->NO, K = g->K;
    double *part_rr = d->part + kPartMax, *tail_rr = g->dist + NO;
    const unsigned ug = ds_upd_grid(NO);
    k_gr_update<true><<<ug, 256, 0, st>>>(scal, nullptr, x, r, p, q, NO, K, part_rr, tail_rr, flags);
    k_gr_rr<<<1, 256, 0, st>>>(part_rr, (int)ug, tail_rr, scal, flags);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_ground_dist_direction(comap_ground *g, double *scal, double *p, const double *r,
                                                    int32_t *flags)
{
    if (!g || !scal || !p || !r || !flags) return -1;
    COMAP_DEVICE_GUARD(g->ctx);
    comap_ctx *ctx = g->ctx;
    k_gr_direction<true><<<grid_for(g->NO), 256, 0, ctx->stream>>>(scal, nullptr, 0, nullptr, p, r, g->NO, g->K, flags);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}
