// destriper_cg.hip -- the destriper's operator and CG on a problem built by destriper_setup.hip:
// the bin, projection (CSR and sliced-ELLPACK), dot, update, direction and map kernels with
// their launchers; comap_destripe_destroy and the accessors; the per-piece C ABI (bin, project,
// dot, cg_*, dist_*, offsets_natural, div_map); comap_destripe_solve.  Layouts: destriper_internal.h.
#include "destriper_internal.h"

namespace {

constexpr int kUpdBlocks = 1024;  // CG update grid cap: its r.r partials are re-summed by every direction block
constexpr int kDirBlocks = 1024;  // CG direction grid cap

// Device-side CG stop flags: flags[0] (every band stopped) makes every kernel of the
// remaining enqueued iterations return at once, so iterations run as replayed
// hipGraph batches with one host round trip per batch; flags[2+b] freezes band b.
__device__ __forceinline__ bool cg_done(const int32_t *flags) { return flags && flags[0]; }
__device__ __forceinline__ bool band_stopped(const int32_t *flags, int b) { return flags && flags[2 + b]; }

// block_final_sum for NB bands at once (band b's partials at part + b kPartMax): the
// same per-band order and result, with every band's loads in flight together.
// red: 4 NB doubles.
template <int NB>
__device__ __forceinline__ void block_final_sums(const double *__restrict__ part, int n, double *red, double (&out)[NB],
                                                 int64_t stride = kPartMax)
{
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    constexpr int kB = 4;
    int i = threadIdx.x;
    for (; i + (kB - 1) * 256 < n; i += kB * 256) {
        double v[NB][kB];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < kB; ++k) v[b][k] = part[(int64_t)b * stride + i + k * 256];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < kB; ++k) acc[b] += v[b][k];
    }
    for (; i < n; i += 256) {
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] += part[(int64_t)b * stride + i];
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = wave_sum(acc[b]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) red[4 * b + (threadIdx.x >> 6)] = acc[b];
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) out[b] = (red[4 * b] + red[4 * b + 1]) + (red[4 * b + 2] + red[4 * b + 3]);
}

// Partial slots [used, stride) of every band set to 0 (by one block).  The multi-rank
// partial buffers (stride kDistParts) are all-reduced in place, so a rank whose grid
// is smaller than another's must clear the slots it does not write each time.
template <int NB>
__device__ __forceinline__ void zero_tail(double *__restrict__ part, int64_t stride, int64_t used)
{
    for (int64_t t = used + threadIdx.x; t < stride; t += blockDim.x)
#pragma unroll
        for (int b = 0; b < NB; ++b) part[(int64_t)b * stride + t] = 0.0;
}

// block_partial of NB accumulators with one pair of barriers; band b's partial goes to
// part[b kPartMax] (same value as block_partial per band).  red: 4 NB doubles.
template <int NB>
__device__ __forceinline__ void block_partials(double (&acc)[NB], double *red, double *part, int64_t stride = kPartMax)
{
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = wave_sum(acc[b]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) red[4 * b + (threadIdx.x >> 6)] = acc[b];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            part[(int64_t)b * stride] = (red[4 * b] + red[4 * b + 1]) + (red[4 * b + 2] + red[4 * b + 3]);
    }
}

// x_out[perm[k]] = x[k] per band (internal offset order -> the caller's)
template <int NB>
__global__ void k_unpermute(const double *__restrict__ x, const int32_t *__restrict__ perm, int64_t NO,
                            double *__restrict__ out)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < NO; k += (int64_t)gridDim.x * blockDim.x) {
        double v[NB];
        ldb<NB>(x + k * NB, v);
        stb<NB>(out + (int64_t)perm[k] * NB, v);
    }
}

// xs = wbar o x per band (the count form's bin input); gated by the CG stop flags
template <int NB>
__global__ void k_scale(const double *__restrict__ wbar, const double *__restrict__ x, int64_t NO,
                        double *__restrict__ xs, const int32_t *__restrict__ flags)
{
    if (cg_done(flags)) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < NO; i += (int64_t)gridDim.x * blockDim.x) {
        double a[NB], v[NB];
        ldb<NB>(wbar + i * NB, a);
        ldb<NB>(x + i * NB, v);
#pragma unroll
        for (int b = 0; b < NB; ++b) v[b] *= a[b];
        stb<NB>(xs + i * NB, v);
    }
}

// The map pixel a projection entry gathers: op_Z reads m[pointing] (Destriper.py:206-213),
// so an unbinned sample's negative id p in [-npix, -1] reads m[npix + p] -- numpy's index
// wrap (-1: the last pixel).  The set-up rejects p < -npix (numpy's IndexError).
__device__ __forceinline__ int64_t wrap_pixel(int32_t p, int64_t npix) { return p >= 0 ? (int64_t)p : npix + p; }

__device__ __forceinline__ double map_value(const double *num, const double *h, int64_t q)
{
    const double hv = h[q];
    return hv != 0.0 ? num[q] / hv : num[q];
}

// num_p = sum_e s_e x_o(e) per band; base != NULL: num = base - W x (final destriped
// numerator); hdiv != NULL: num = m = (W x) / h, the map itself (single rank: k_ds_project
// then gathers one array).  kBinLanes lanes per pixel row (rows hold 0 .. thousands of
// entries), lane-strided; each lane issues kBinU entry loads, then kBinU gathers of the
// NB-band x vectors, before its fmas (in entry order, so the sum is the plain
// lane-strided one), then a kBinLanes-lane reduction.
template <int kBinLanes, int NB, bool CF, int kBinU>
__global__ void __launch_bounds__(256) k_ds_bin(const int64_t *__restrict__ prow, const int32_t *__restrict__ poff,
                                                const void *__restrict__ pw, const double *__restrict__ x,
                                                int64_t npix, const double *__restrict__ base,
                                                const double *__restrict__ hdiv, double *__restrict__ num,
                                                const int32_t *__restrict__ flags, const int32_t *__restrict__ rows)
{
    if (cg_done(flags)) return;
    const int sub = threadIdx.x & (kBinLanes - 1);
    const int64_t step = (int64_t)gridDim.x * blockDim.x / kBinLanes;
    // rows != NULL: only the listed (non-empty) rows, npix = their count, and prow holds
    // their entry ranges (hprow: row i spans [prow[i], prow[i + 1]), no dependent row load)
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kBinLanes; i < npix; i += step) {
        const int64_t p = rows ? (int64_t)rows[i] : i;
        double s[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) s[b] = 0.0;
        // the row's base / h values, loaded by the lead lane up front (their latency
        // overlaps the row's gathers instead of following its reduction)
        double tail[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) tail[b] = 0.0;
        if (sub == 0 && (base || hdiv)) ldb<NB>((base ? base : hdiv) + p * NB, tail);
        const int64_t e1 = prow[i + 1];
        // software pipeline: the next group's entry loads are issued before this group's
        // x gathers are consumed, so a lane has one dependent latency per group, not two
        int64_t k = prow[i] + sub;
        int32_t o[kBinU];
        Coef<NB, CF> a[kBinU];
#pragma unroll
        for (int u = 0; u < kBinU; ++u) {
            const bool in = k + u * kBinLanes < e1;
            o[u] = in ? poff[k + u * kBinLanes] : 0;
            if (in) a[u].load(pw, k + u * kBinLanes);
        }
        while (k < e1) {
            double xv[kBinU][NB];
#pragma unroll
            for (int u = 0; u < kBinU; ++u) ldb<NB>(x + (int64_t)o[u] * NB, xv[u]);
            const int64_t kn = k + kBinLanes * kBinU;
            int32_t on[kBinU];
            Coef<NB, CF> an[kBinU];
#pragma unroll
            for (int u = 0; u < kBinU; ++u) {
                const bool in = kn + u * kBinLanes < e1;
                on[u] = in ? poff[kn + u * kBinLanes] : 0;
                if (in) an[u].load(pw, kn + u * kBinLanes);
            }
#pragma unroll
            for (int u = 0; u < kBinU; ++u)
                if (k + u * kBinLanes < e1) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) s[b] = fma(a[u].get(b), xv[u][b], s[b]);
                }
#pragma unroll
            for (int u = 0; u < kBinU; ++u) { o[u] = on[u]; a[u] = an[u]; }
            k = kn;
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int o = kBinLanes / 2; o > 0; o >>= 1) s[b] += __shfl_xor(s[b], o, kBinLanes);
        }
        if (sub == 0) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (base) s[b] = tail[b] - s[b];
                else if (hdiv) { const double hv = tail[b]; s[b] = hv != 0.0 ? s[b] / hv : s[b]; }
            }
            stb<NB>(num + p * NB, s);
        }
    }
}

// y_o = ws_o x_o - sum_e s_e m_p(e) per band  (x == NULL: y_o = tw_o - ..., the b vector).
// G lanes per offset (G = 16 for L <= 64: 256/G offsets per block sweep); each lane issues
// kProjU entry loads then kProjU map gathers before its fmas; m = num / h, or num itself
// when h == NULL (k_ds_bin already divided).  Block partials of y.x per band
// (dot_part + b kPartMax, when dot_part != NULL).
template <int G, int NB, bool CF, int kProjU>
__global__ void __launch_bounds__(256) k_ds_project(const int64_t *__restrict__ orow, const int32_t *__restrict__ opix,
                                                    const void *__restrict__ ow, const double *__restrict__ wbar,
                                                    const double *__restrict__ ws,
                                                    const double *__restrict__ tw, const double *__restrict__ x,
                                                    const double *__restrict__ num, const double *__restrict__ h,
                                                    int64_t NO, int64_t npix, double *__restrict__ y,
                                                    double *__restrict__ dot_part, const int32_t *__restrict__ flags,
                                                    int64_t pstride = kPartMax)
{
    __shared__ double red[4 * NB];
    if (cg_done(flags)) return;
    constexpr int kPer = 256 / G;
    const int sub = threadIdx.x & (G - 1);
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    // Software pipeline over the block's sweeps (kPer offsets each): while this sweep's
    // map gathers are in flight, the next sweep's first pass of entries (and the row
    // bounds of the one after) are already being loaded -- a lane waits on one dependent
    // latency per sweep instead of three.  Rows longer than one pass (G kProjU entries)
    // finish with plain passes.
    const int64_t stride = (int64_t)gridDim.x * kPer;
    int64_t o = (int64_t)blockIdx.x * kPer + threadIdx.x / G;
    int64_t b0 = 0, b1 = 0, nb0 = 0, nb1 = 0;
    if (o < NO) { b0 = orow[o]; b1 = orow[o + 1]; }
    if (o + stride < NO) { nb0 = orow[o + stride]; nb1 = orow[o + stride + 1]; }
    int32_t cq[kProjU];
    Coef<NB, CF> ca[kProjU];
    auto load_pass = [&](int64_t e, int64_t e1, int32_t (&q)[kProjU], Coef<NB, CF> (&a)[kProjU]) {
#pragma unroll
        for (int u = 0; u < kProjU; ++u) {
            const bool in = e + u * G < e1;
            q[u] = in ? (int32_t)wrap_pixel(opix[e + u * G], npix) : 0;   // numpy's m[p] wrap for p < 0
            if (in) a[u].load(ow, e + u * G);
            else a[u] = Coef<NB, CF>();
        }
    };
    auto gather = [&](const int32_t (&q)[kProjU], double (&mv)[kProjU][NB]) {
#pragma unroll
        for (int u = 0; u < kProjU; ++u) {
            if (h) {
#pragma unroll
                for (int b = 0; b < NB; ++b) mv[u][b] = map_value(num, h, (int64_t)q[u] * NB + b);
            } else {
                ldb<NB>(num + (int64_t)q[u] * NB, mv[u]);
            }
        }
    };
    load_pass(b0 + sub, b1, cq, ca);
    for (; o - threadIdx.x / G < NO; o += stride) {
        const bool valid = o < NO;
        const int64_t e0 = b0, e1 = b1;
        double g[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) g[b] = 0.0;
        double mv[kProjU][NB];
        gather(cq, mv);
        // next sweep: its first pass of entries, and the row bounds of the sweep after it
        int32_t nq[kProjU];
        Coef<NB, CF> na[kProjU];
        load_pass(nb0 + sub, nb1, nq, na);
        b0 = nb0; b1 = nb1;
        nb0 = nb1 = 0;
        if (o + 2 * stride < NO) { nb0 = orow[o + 2 * stride]; nb1 = orow[o + 2 * stride + 1]; }
#pragma unroll
        for (int u = 0; u < kProjU; ++u)
            if (e0 + sub + u * G < e1) {
#pragma unroll
                for (int b = 0; b < NB; ++b) g[b] = fma(ca[u].get(b), mv[u][b], g[b]);
            }
        for (int64_t e = e0 + sub + G * kProjU; e < e1; e += G * kProjU) {   // long rows
            int32_t q[kProjU];
            Coef<NB, CF> a[kProjU];
            load_pass(e, e1, q, a);
            double mw[kProjU][NB];
            gather(q, mw);
#pragma unroll
            for (int u = 0; u < kProjU; ++u)
                if (e + u * G < e1) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) g[b] = fma(a[u].get(b), mw[u][b], g[b]);
                }
        }
#pragma unroll
        for (int u = 0; u < kProjU; ++u) { cq[u] = nq[u]; ca[u] = na[u]; }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int s = G / 2; s > 0; s >>= 1) g[b] += __shfl_xor(g[b], s, G);
        }
        if (valid && sub == 0) {
            // (loading x / wbar / ws at the top of the sweep, beside the gathers, measured
            // slower: 124.6 -> 136.4 us at C5 4 bands, r03t4)
            double xo[NB], v[NB];
            if (x) {
                ldb<NB>(x + o * NB, xo);
            } else {
#pragma unroll
                for (int b = 0; b < NB; ++b) xo[b] = 0.0;
            }
            if constexpr (CF) {   // the row's sum of counts x m, times the offset's weight
                double wb[NB];
                ldb<NB>(wbar + o * NB, wb);
#pragma unroll
                for (int b = 0; b < NB; ++b) g[b] *= wb[b];
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                v[b] = (x ? ws[o * NB + b] * xo[b] : tw[o * NB + b]) - g[b];
                if (dot_part) acc[b] = fma(v[b], xo[b], acc[b]);
            }
            stb<NB>(y + o * NB, v);
        }
    }
    if (dot_part) {
        block_partials<NB>(acc, red, dot_part + blockIdx.x, pstride);
        if (pstride < kPartMax && blockIdx.x == 0) zero_tail<NB>(dot_part, pstride, gridDim.x);
    }
}

// ---------------------------------------------------------------- sliced-ELLPACK projection
// k_ds_project on the sliced-ELLPACK rows: one wave per chunk of 64 offsets (chunks dealt
// to the grid's waves round-robin), lane = offset.  Each lane walks its row in groups of U
// entries: the group's pixel ids and coefficients are coalesced loads issued one group
// ahead of its map gathers, and the row sum is a plain in-order fma chain per lane (no
// shuffles).  Same outputs as k_ds_project (y, block partials of y.x per band).
template <int NB, bool CF, int U>
__global__ void __launch_bounds__(256) k_ds_project_sell(const int64_t *__restrict__ sbase,
                                                         const int32_t *__restrict__ spix, const void *__restrict__ sco,
                                                         const double *__restrict__ wbar, const double *__restrict__ ws,
                                                         const double *__restrict__ tw, const double *__restrict__ x,
                                                         const double *__restrict__ num, const double *__restrict__ h,
                                                         int64_t NO, int64_t npix, double *__restrict__ y,
                                                         double *__restrict__ dot_part, const int32_t *__restrict__ flags,
                                                         int64_t pstride)
{
    __shared__ double red[4 * NB];
    if (cg_done(flags)) return;
    const int lane = threadIdx.x & 63;
    const int64_t NC = (NO + 63) >> 6;
    const int64_t nw = (int64_t)gridDim.x * 4;
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < NC; c += nw) {
        const int64_t b0 = sbase[c], W = (sbase[c + 1] - b0) >> 6;
        const int64_t o = c * 64 + lane;
        const int32_t *pp = spix + b0 + lane;
        double g[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) g[b] = 0.0;
        int32_t q[U];
        Coef<NB, CF> a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = u < W;
            q[u] = in ? pp[64 * u] : kSellPad;
            if (in) a[u].load(sco, b0 + 64 * u + lane);
        }
        for (int64_t j = 0; j < W; j += U) {
            double mv[U][NB];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (q[u] != kSellPad) {
                    const int64_t qq = wrap_pixel(q[u], npix);     // m[p] with numpy's wrap for p < 0
                    if (h) {
#pragma unroll
                        for (int b = 0; b < NB; ++b) mv[u][b] = map_value(num, h, qq * NB + b);
                    } else {
                        ldb<NB>(num + qq * NB, mv[u]);
                    }
                }
            }
            const int64_t jn = j + U;
            int32_t qn[U];
            Coef<NB, CF> an[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = jn + u < W;
                qn[u] = in ? pp[64 * (jn + u)] : kSellPad;
                if (in) an[u].load(sco, b0 + 64 * (jn + u) + lane);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (q[u] != kSellPad) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) g[b] = fma(a[u].get(b), mv[u][b], g[b]);
                }
#pragma unroll
            for (int u = 0; u < U; ++u) { q[u] = qn[u]; a[u] = an[u]; }
        }
        if (o < NO) {
            double v[NB], xo[NB], wb[NB], wsv[NB];
            if (x) ldb<NB>(x + o * NB, xo);
            if constexpr (CF) ldb<NB>(wbar + o * NB, wb);
            ldb<NB>((x ? ws : tw) + o * NB, wsv);
            if (!x) {
#pragma unroll
                for (int b = 0; b < NB; ++b) xo[b] = 0.0;
            }
            if constexpr (CF) {
#pragma unroll
                for (int b = 0; b < NB; ++b) g[b] *= wb[b];
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                v[b] = (x ? wsv[b] * xo[b] : wsv[b]) - g[b];
                if (dot_part) acc[b] = fma(v[b], xo[b], acc[b]);
            }
            stb<NB>(y + o * NB, v);
        }
    }
    if (dot_part) {
        block_partials<NB>(acc, red, dot_part + blockIdx.x, pstride);
        if (pstride < kPartMax && blockIdx.x == 0) zero_tail<NB>(dot_part, pstride, gridDim.x);
    }
}

// per-band block partials of sum_o a[o][b] c[o][b]
template <int NB>
__global__ void __launch_bounds__(256) k_dot_part(const double *__restrict__ a, const double *__restrict__ c, int64_t n,
                                                  double *__restrict__ part)
{
    __shared__ double red[4 * NB];
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double av[NB], cv[NB];
        ldb<NB>(a + i * NB, av);
        ldb<NB>(c + i * NB, cv);
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = fma(av[b], cv[b], acc[b]);
    }
    block_partials<NB>(acc, red, part + blockIdx.x);
}

// out[b] = fixed-order sum of band b's n partials
template <int NB>
__global__ void __launch_bounds__(256) k_dot_final(const double *__restrict__ part, int n, double *__restrict__ out,
                                                   const int32_t *__restrict__ flags)
{
    __shared__ double red[4];
    if (cg_done(flags)) return;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const double sum = block_final_sum(part + (int64_t)b * kPartMax, n, red);
        if (threadIdx.x == 0) out[b] = sum;
    }
}

// x += a p ; r -= a q ; a = rr / pq per band (bands already stopped are left alone);
// per-band partials of r.r
template <int NB>
__global__ void __launch_bounds__(256) k_cg_update(const double *__restrict__ rr, const double *__restrict__ pq,
                                                   double *__restrict__ x, double *__restrict__ r,
                                                   const double *__restrict__ p, const double *__restrict__ q,
                                                   int64_t n, double *__restrict__ part, const int32_t *__restrict__ flags)
{
    __shared__ double red[4 * NB];
    if (cg_done(flags)) return;
    double a[NB], acc[NB];
    bool live[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { a[b] = rr[b] / pq[b]; live[b] = !band_stopped(flags, b); acc[b] = 0.0; }
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        update_row<NB>(x + i * NB, r + i * NB, p + i * NB, q + i * NB, a, live, acc);
    block_partials<NB>(acc, red, part + blockIdx.x);
}

// End-of-iteration bookkeeping (Destriper.py:136-152) by one thread, per band still
// running: rr = rr_new, count it, stop when delta = rr_new / rr0 is NaN or below the
// threshold; flags[1] counts iterations any band ran, flags[0] = every band stopped.
template <int NB>
__device__ __forceinline__ void cg_check(double *__restrict__ scal, int32_t *__restrict__ flags, const double *rrn)
{
    bool any = false, all = true;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (!flags[2 + b]) {
            any = true;
            scal[3 * NB + b] = rrn[b];
            flags[2 + NB + b] += 1;
            const double delta = rrn[b] / scal[b];
            if (isnan(delta) || delta < scal[4 * NB]) flags[2 + b] = 1;
        }
        all = all && flags[2 + b];
    }
    if (any) flags[1] += 1;
    if (all) flags[0] = 1;
}

// Fused single-rank CG tail (comap_destripe_solve): no separate final-sum or check
// launches.  Every block re-derives the global sums from the previous kernel's block
// partials in k_dot_final's order, so all blocks hold identical values and no block
// waits on another.  Per band: scal[b] rr0, scal[NB+b] rr of this iteration (for beta),
// scal[3NB+b] current rr.
//   k_cg_update_fused: pq = sum(pq partials); a = rr / pq; x += a p; r -= a q;
//                      r.r partials into part_rr; block 0 saves rr and pq
//   k_cg_direction_fused: rr_new = sum(part_rr); p = r + (rr_new / rr) p;
//                      block 0: rr = rr_new, count, stop test (cg_check)
template <int NB>
__global__ void __launch_bounds__(256) k_cg_update_fused(double *__restrict__ scal, const double *__restrict__ part_pq,
                                                         int npq, double *__restrict__ x, double *__restrict__ r,
                                                         const double *__restrict__ p, const double *__restrict__ q,
                                                         int64_t n, double *__restrict__ part_rr,
                                                         const int32_t *__restrict__ flags, int64_t pstride = kPartMax)
{
    __shared__ double red[4 * NB];
    if (cg_done(flags)) return;
    double pq[NB], rr[NB], a[NB], acc[NB];
    bool live[NB];
    block_final_sums<NB>(part_pq, npq, red, pq, pstride);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        rr[b] = scal[3 * NB + b];
        a[b] = rr[b] / pq[b];
        live[b] = !band_stopped(flags, b);
        acc[b] = 0.0;
    }
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        update_row<NB>(x + i * NB, r + i * NB, p + i * NB, q + i * NB, a, live, acc);
    block_partials<NB>(acc, red, part_rr + blockIdx.x, pstride);
    if (pstride < kPartMax && blockIdx.x == 0) zero_tail<NB>(part_rr, pstride, gridDim.x);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (live[b]) { scal[NB + b] = rr[b]; scal[2 * NB + b] = pq[b]; }
    }
}

template <int NB>
__global__ void __launch_bounds__(256) k_cg_direction_fused(double *__restrict__ scal, const double *__restrict__ part_rr,
                                                            int nrr, double *__restrict__ p, const double *__restrict__ r,
                                                            int64_t n, int32_t *flags, int64_t pstride = kPartMax,
                                                            const double *__restrict__ wbar = nullptr,
                                                            double *__restrict__ pt = nullptr)
{
    __shared__ double red[4 * NB];
    if (flags[0]) return;
    double rrn[NB], beta[NB];
    bool live[NB];
    block_final_sums<NB>(part_rr, nrr, red, rrn, pstride);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        beta[b] = rrn[b] / scal[NB + b];
        live[b] = !flags[2 + b];
    }
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        direction_row<NB>(p + i * NB, r + i * NB, beta, live, wbar ? wbar + i * NB : nullptr,
                          wbar ? pt + i * NB : nullptr);
    // block 0 only, after its own sweep: a band that stops here never reads p again.
    // scal[NB+b] is left alone -- other blocks may still be reading it for beta; the
    // fused update takes rr from scal[3NB+b] and rewrites scal[NB+b] itself.
    if (blockIdx.x == 0 && threadIdx.x == 0) cg_check<NB>(scal, flags, rrn);
}

// p = r + (rr_new / rr) p per band still running
template <int NB>
__global__ void k_cg_direction(const double *__restrict__ rr_new, const double *__restrict__ rr, double *__restrict__ p,
                               const double *__restrict__ r, int64_t n, const int32_t *__restrict__ flags)
{
    if (cg_done(flags)) return;
    double beta[NB];
    bool live[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { beta[b] = rr_new[b] / rr[b]; live[b] = !band_stopped(flags, b); }
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        direction_row<NB>(p + i * NB, r + i * NB, beta, live);
}

__global__ void k_div_map(const double *__restrict__ num, const double *__restrict__ h, int64_t n,
                          double *__restrict__ out)
{
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x)
        out[p] = map_value(num, h, p);
}

// CG update grid: one offset row per thread up to kUpdBlocks blocks (the fused and the
// per-piece paths use the same grid, hence the same r.r partials)
inline unsigned upd_grid(int64_t NO) { return grid_for(NO, kUpdBlocks); }

// k_ds_bin with kBinLanes sized to the mean pixel-row length (sparse C4-like maps
// hold ~5 entries per pixel: 16 lanes per row would leave most lanes idle and
// need several latency-bound grid sweeps); one sweep over all rows.
// hit_rows: only the non-empty rows (d->hrow; the caller's num must hold 0 on the
// empty rows, as the CG's own map buffer does).  Count form: x must already be
// scaled (wbar o x, x_scaled) or is scaled into d->pt first.
template <int NB, bool CF, int U>
void launch_bin_u(const comap_destriper *d, hipStream_t st, const double *x, const double *base, const double *hdiv,
                  double *num, const int32_t *flags, bool hit_rows)
{
    const int64_t np = hit_rows ? d->nh : d->npix;
    const int32_t *rows = hit_rows ? d->hrow : nullptr;
    const int64_t *rp = hit_rows ? d->hprow : d->prow;
    const int64_t mean = np ? d->nnzp / np : 0;
    const void *co = CF ? (const void *)d->pcnt : (const void *)d->pw;
    // (rows of >= 256 entries -- the field's 415 -- with 8 loads per lane: 32 lanes, field 4 bands
    // 1.354 -> 1.336 ms, 1 band 0.655 -> 0.623 ms per iteration, profiles/r06/r06cg)
    const int lanes = d->opt.bin_lanes ? d->opt.bin_lanes
                                   : (mean >= 256 && U == 8 ? 32 : (mean >= 24 ? 16 : (mean >= 10 ? 8 : 4)));
    const unsigned g = grid_for(np * lanes, 65536);
#define COMAP_BIN(LN) k_ds_bin<LN, NB, CF, U><<<g, 256, 0, st>>>(rp, d->poff, co, x, np, base, hdiv, num, flags, rows)
    switch (lanes) {
    case 64: COMAP_BIN(64); break;
    case 32: COMAP_BIN(32); break;
    case 16: COMAP_BIN(16); break;
    case 8: COMAP_BIN(8); break;
    default: COMAP_BIN(4);
    }
#undef COMAP_BIN
}

template <int NB, bool CF>
void launch_bin_cf(const comap_destriper *d, hipStream_t st, const double *x, const double *base, const double *hdiv,
                   double *num, const int32_t *flags, bool hit_rows)
{
    if (d->bin_u == 8) launch_bin_u<NB, CF, 8>(d, st, x, base, hdiv, num, flags, hit_rows);
    else launch_bin_u<NB, CF, 4>(d, st, x, base, hdiv, num, flags, hit_rows);
}

void launch_bin(const comap_destriper *d, hipStream_t st, const double *x, const double *base, const double *hdiv,
                double *num, const int32_t *flags, bool hit_rows = false, bool x_scaled = false)
{
    if (d->cf && !x_scaled) {
        COMAP_NB_SWITCH(d->nb, k_scale<NB><<<grid_for(d->NO), 256, 0, st>>>(d->wbar, x, d->NO, d->pt, flags));
        x = d->pt;
    }
    if (d->cf) {
        COMAP_NB_SWITCH(d->nb, (launch_bin_cf<NB, true>(d, st, x, base, hdiv, num, flags, hit_rows)));
    } else {
        COMAP_NB_SWITCH(d->nb, (launch_bin_cf<NB, false>(d, st, x, base, hdiv, num, flags, hit_rows)));
    }
}

// lanes per offset row: the fewest whose one pass of kProjU loads covers the mean row
// (C5: 28 entries per offset -> 8 lanes, 32 offsets per block sweep; C4: 14 -> 4).
// Measured at C5 (r03e, ms per CG iteration, 1 / 4 bands): 16 lanes 0.152 / 0.347,
// 8 lanes 0.132 / 0.307; 8 loads per lane or a 2048-block grid: within noise or slower.
inline int project_lanes(const comap_destriper *d)
{
    if (d->opt.proj_lanes) return d->opt.proj_lanes;
    const int64_t mean = d->NO ? (d->nnz + d->NO - 1) / d->NO : 0;
    int g = 4;
    while (g < 64 && g * kProjU < mean) g *= 2;
    return g;
}
inline unsigned project_grid(const comap_destriper *d, int64_t cap)
{
    const int64_t per = d->sell ? 256 : 256 / project_lanes(d);   // offsets per block sweep
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((d->NO + per - 1) / per, std::min<int64_t>(cap, d->proj_blocks)));
}

// k_ds_project with the lane group sized to the offset length; returns its grid (= partials).
template <int NB, bool CF>
unsigned launch_project_cf(const comap_destriper *d, hipStream_t st, const double *x, const double *num,
                           const double *h, double *y, double *part, const int32_t *flags, int64_t pstride)
{
    const unsigned pg = project_grid(d, pstride);
    if (d->sell) {
        k_ds_project_sell<NB, CF, 8><<<pg, 256, 0, st>>>(d->sbase, d->spix, d->sco, d->wbar, d->ws, d->tw, x, num, h,
                                                        d->NO, d->npix, y, part, flags, pstride);
        return pg;
    }
    const void *co = CF ? (const void *)d->ocnt : (const void *)d->ow;
#define COMAP_PROJ(G) k_ds_project<G, NB, CF, kProjU><<<pg, 256, 0, st>>>(d->orow, d->opix, co, d->wbar, d->ws, d->tw, \
                                                                          x, num, h, d->NO, d->npix, y, part, flags, \
                                                                          pstride)
    switch (project_lanes(d)) {
    case 4: COMAP_PROJ(4); break;
    case 8: COMAP_PROJ(8); break;
    case 16: COMAP_PROJ(16); break;
    case 32: COMAP_PROJ(32); break;
    default: COMAP_PROJ(64);
    }
#undef COMAP_PROJ
    return pg;
}

unsigned launch_project(const comap_destriper *d, hipStream_t st, const double *x, const double *num,
                        const double *h, double *y, double *part, const int32_t *flags, int64_t pstride = kPartMax)
{
    unsigned pg = 0;
    if (d->cf) {
        COMAP_NB_SWITCH(d->nb, (pg = launch_project_cf<NB, true>(d, st, x, num, h, y, part, flags, pstride)));
    } else {
        COMAP_NB_SWITCH(d->nb, (pg = launch_project_cf<NB, false>(d, st, x, num, h, y, part, flags, pstride)));
    }
    return pg;
}

int dot(comap_destriper *d, hipStream_t st, const double *a, const double *b, double *out, const int32_t *flags)
{
    comap_ctx *ctx = d->ctx;
    COMAP_NB_SWITCH(d->nb, k_dot_part<NB><<<kRedBlocks, 256, 0, st>>>(a, b, d->NO, d->part);
                    k_dot_final<NB><<<1, 256, 0, st>>>(d->part, kRedBlocks, out, flags));
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

}  // namespace

// ---- the launchers the ground solve shares (declared in destriper_internal.h; one band)
void ds_launch_bin(const comap_destriper *d, hipStream_t st, const double *x, const double *base, const double *hdiv,
                   double *num, const int32_t *flags, bool hit_rows, bool x_scaled)
{
    launch_bin(d, st, x, base, hdiv, num, flags, hit_rows, x_scaled);
}

void ds_launch_project(const comap_destriper *d, hipStream_t st, const double *x, const double *num, const double *h,
                       double *y, const int32_t *flags)
{
    launch_project(d, st, x, num, h, y, nullptr, flags);
}

void ds_dot(comap_destriper *d, hipStream_t st, const double *a, const double *b, int64_t n, double *out)
{
    k_dot_part<1><<<kRedBlocks, 256, 0, st>>>(a, b, n, d->part);
    k_dot_final<1><<<1, 256, 0, st>>>(d->part, kRedBlocks, out, nullptr);
}

void ds_dot_part(comap_destriper *d, hipStream_t st, const double *a, const double *b, int64_t n)
{
    k_dot_part<1><<<kRedBlocks, 256, 0, st>>>(a, b, n, d->part);
}

unsigned ds_upd_grid(int64_t NO) { return upd_grid(NO); }

// ---- the native solve's own launches as the prior solve (destriper_prior.hip) enqueues them
unsigned ds_launch_project_parts(const comap_destriper *d, hipStream_t st, const double *x, const double *num,
                                 double *y, const int32_t *flags)
{
    return launch_project(d, st, x, num, nullptr, y, d->part, flags);
}

void ds_launch_update_fused(const comap_destriper *d, hipStream_t st, int npq, double *x, double *r, const double *p,
                            const double *q, const int32_t *flags)
{
    k_cg_update_fused<1><<<upd_grid(d->NO), 256, 0, st>>>(d->scal, d->part, npq, x, r, p, q, d->NO, d->part + kPartMax,
                                                          flags);
}

void ds_launch_direction_fused(const comap_destriper *d, hipStream_t st, double *p, const double *r, int32_t *flags)
{
    k_cg_direction_fused<1><<<grid_for(d->NO, kDirBlocks), 256, 0, st>>>(
        d->scal, d->part + kPartMax, (int)upd_grid(d->NO), p, r, d->NO, flags, kPartMax, d->cf ? d->wbar : nullptr,
        d->cf ? d->pt : nullptr);
}

void ds_scale(const comap_destriper *d, hipStream_t st, const double *x, double *xs)
{
    k_scale<1><<<grid_for(d->NO), 256, 0, st>>>(d->wbar, x, d->NO, xs, nullptr);
}

void ds_unpermute(const comap_destriper *d, hipStream_t st, const double *x, double *out)
{
    k_unpermute<1><<<grid_for(d->NO), 256, 0, st>>>(x, d->perm, d->NO, out);
}

void ds_div_map(hipStream_t st, const double *num, const double *h, int64_t n, double *out)
{
    k_div_map<<<grid_for(n), 256, 0, st>>>(num, h, n, out);
}

extern "C" int comap_destripe_destroy(comap_destriper *d)
{
    if (!d) return 0;
    COMAP_DEVICE_GUARD(d->ctx);
    if (d->nviews > 0) return comap_fail(d->ctx, -1, "destroying a problem that still has a live solve-mask view");
    // every stream that may still read the buffers (the CG stream, the caller's) is idle
    // after a device sync; the blocks then go back to the caches
    (void)hipDeviceSynchronize();
    if (d->parent) {   // a solve-mask view: the index structure, wbar and hits are its parent's
        void *b[] = {d->ow, d->ws, d->tw, d->pw, d->h, d->nnum, d->part, d->scal, d->cg, d->flags, d->ocnt, d->pcnt,
                     d->pt, d->sco};
        comap_tmp_free_on(b, (int)(sizeof(b) / sizeof(b[0])), nullptr, true);
        --d->parent->nviews;
    } else {
        void *b[] = {d->orow, d->opix, d->ow, d->ws, d->tw, d->prow, d->poff, d->pw, d->h, d->hits, d->nnum, d->part,
                     d->scal, d->cg, d->flags, d->hrow, d->hprow, d->perm, d->ocnt, d->pcnt, d->wbar, d->pt, d->sbase,
                     d->spix, d->sco};
        comap_tmp_free_on(b, (int)(sizeof(b) / sizeof(b[0])), nullptr, true);
    }
    comap_pinned_free(d->flags_host);
    comap_pinned_free(d->thr_host);
    if (d->batch) (void)hipGraphExecDestroy(d->batch);
    if (d->ev) (void)hipEventDestroy(d->ev);
    comap_stream_release(d->cs);
    delete d;
    return 0;
}

extern "C" int64_t comap_destripe_n_offsets(const comap_destriper *d) { return d ? d->NO : -1; }
extern "C" int32_t comap_destripe_n_bands(const comap_destriper *d) { return d ? d->nb : -1; }

extern "C" int64_t comap_destripe_sell_entries(const comap_destriper *d) { return d && d->sell ? d->nsell : -1; }

extern "C" int32_t comap_destripe_entry_bytes(const comap_destriper *d)
{
    return d ? (d->cf ? 4 + d->nb : 4 + 8 * d->nb) : -1;
}

extern "C" int comap_destripe_nnz(const comap_destriper *d, int64_t *nnz_offset_major, int64_t *nnz_pixel_major)
{
    if (!d) return -1;
    if (nnz_offset_major) *nnz_offset_major = d->nnz;
    if (nnz_pixel_major) *nnz_pixel_major = d->nnzp;
    return 0;
}

extern "C" int comap_destripe_local_maps(comap_destriper *d, double *h, double *hits, double *naive_num)
{
    if (!d) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    const size_t b = 8 * (size_t)d->npix * d->nb;
    if (h) COMAP_CHECK(ctx, hipMemcpyAsync(h, d->h, b, hipMemcpyDeviceToDevice, ctx->stream));
    if (hits) COMAP_CHECK(ctx, hipMemcpyAsync(hits, d->hits, b, hipMemcpyDeviceToDevice, ctx->stream));
    if (naive_num) COMAP_CHECK(ctx, hipMemcpyAsync(naive_num, d->nnum, b, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

extern "C" int comap_destripe_bin(comap_destriper *d, const double *x, int32_t mode, double *num)
{
    if (!d || !x || !num) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    launch_bin(d, ctx->stream, x, mode == 1 ? d->nnum : nullptr, nullptr, num, nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_project(comap_destriper *d, const double *x, const double *num, const double *h,
                                      double *y, double *dot_out)
{
    if (!d || !num || !y) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    const double *hh = h ? h : d->h;
    const bool want = dot_out && x;
    const unsigned pg = launch_project(d, ctx->stream, x, num, hh, y, want ? d->part : nullptr, nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    if (want) {
        COMAP_NB_SWITCH(d->nb, k_dot_final<NB><<<1, 256, 0, ctx->stream>>>(d->part, (int)pg, dot_out, nullptr));
        COMAP_LAUNCH_CHECK(ctx);
    }
    return 0;
}

extern "C" int comap_destripe_dot(comap_destriper *d, const double *a, const double *b, double *out)
{
    if (!d || !a || !b || !out) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    return dot(d, d->ctx->stream, a, b, out, nullptr);
}

extern "C" int comap_destripe_cg_update(comap_destriper *d, const double *rr, const double *pq, double *x, double *r,
                                        const double *p, const double *q, double *rr_new)
{
    if (!d) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    COMAP_NB_SWITCH(d->nb, k_cg_update<NB><<<upd_grid(d->NO), 256, 0, ctx->stream>>>(rr, pq, x, r, p, q, d->NO, d->part,
                                                                                 nullptr);
                    k_dot_final<NB><<<1, 256, 0, ctx->stream>>>(d->part, (int)upd_grid(d->NO), rr_new, nullptr));
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_cg_direction(comap_destriper *d, const double *rr_new, const double *rr, double *p,
                                           const double *r)
{
    if (!d) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    COMAP_NB_SWITCH(d->nb, k_cg_direction<NB><<<grid_for(d->NO), 256, 0, ctx->stream>>>(rr_new, rr, p, r, d->NO,
                                                                                         nullptr));
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_offsets_natural(comap_destriper *d, const double *x_internal, double *x_out)
{
    if (!d || !x_internal || !x_out || x_internal == x_out) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    COMAP_NB_SWITCH(d->nb, k_unpermute<NB><<<grid_for(d->NO), 256, 0, ctx->stream>>>(x_internal, d->perm, d->NO, x_out));
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_div_map(comap_destriper *d, const double *num, const double *h, double *out)
{
    if (!d || !num || !out) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    const int64_t n = d->npix * d->nb;
    k_div_map<<<grid_for(n), 256, 0, ctx->stream>>>(num, h ? h : d->h, n, out);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

// ---------------------------------------------------------------- multi-rank CG pieces
// One CG iteration split at its three all-reduce points (map numerator, p.q,
// r.r), every kernel gated by the device stop flags so the host can queue a
// batch of iterations (with the collectives between the pieces) and check the
// flags once per batch.  Scalar / flag layout: destriper_internal.h.
extern "C" int comap_destripe_dist_bin(comap_destriper *d, const double *p, double *num, const int32_t *flags)
{
    if (!d || !p || !num || !flags) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    launch_bin(d, ctx->stream, p, nullptr, nullptr, num, flags);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

// The rest of the iteration is the native solve's kernels, with the p.q and r.r block
// partials (one slot per block, kDistParts per band, zero beyond the grid) all-reduced
// between them.  Adding the zero slots changes no bit, so on one rank the iterates equal
// comap_destripe_solve's -- as long as the projection runs the native solve's grid, i.e. the
// slots hold it: 2 kProjBlocks, the sliced-ELLPACK projection's default grid cap below 2 M
// offsets (1024 slots capped its grid from 262 144 offsets on, and the p.q partials, hence
// every iterate, then differed from the native solve's in the last bits).  A problem whose
// projection grid is larger still (2 M offsets and more, COMAP_DS_PB above 2048) runs it on
// kDistParts blocks here.
constexpr int kDistParts = 2 * kProjBlocks;   // >= the default projection grids, kUpdBlocks
static_assert(kDistParts >= 2 * kProjBlocks && kDistParts >= kUpdBlocks && kDistParts <= kPartMax, "partial slots");

extern "C" int32_t comap_destripe_dist_parts(void) { return kDistParts; }

extern "C" int comap_destripe_dist_project_parts(comap_destriper *d, const double *p, const double *num,
                                                 const double *h, double *q, double *pq_part, const int32_t *flags)
{
    if (!d || !p || !num || !h || !q || !pq_part || !flags) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    launch_project(d, ctx->stream, p, num, h, q, pq_part, flags, kDistParts);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_dist_update_fused(comap_destriper *d, double *scal, const double *pq_part, double *x,
                                                double *r, const double *p, const double *q, double *rr_part,
                                                const int32_t *flags)
{
    if (!d || !scal || !pq_part || !x || !r || !p || !q || !rr_part || !flags) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    COMAP_NB_SWITCH(d->nb, k_cg_update_fused<NB><<<upd_grid(d->NO), 256, 0, ctx->stream>>>(
                               scal, pq_part, kDistParts, x, r, p, q, d->NO, rr_part, flags, kDistParts));
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_dist_direction_fused(comap_destriper *d, double *scal, const double *rr_part, double *p,
                                                   const double *r, int32_t *flags)
{
    if (!d || !scal || !rr_part || !p || !r || !flags) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    COMAP_NB_SWITCH(d->nb, k_cg_direction_fused<NB><<<grid_for(d->NO, kDirBlocks), 256, 0, ctx->stream>>>(
                               scal, rr_part, kDistParts, p, r, d->NO, flags, kDistParts));
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

// ---------------------------------------------------------------- device-resident CG
// One CG iteration (Destriper.py:85-152 with p == pb, r == rb) on the problem's own
// vectors for every band; every kernel returns at once after all bands stopped.
static void enqueue_iteration(comap_destriper *d, hipStream_t st)
{
    const int64_t n = d->NO * d->nb;
    double *x = d->cg, *r = x + n, *p = r + n, *q = p + n, *num = q + n;
    const int32_t *flags = d->flags;
    // the bin writes the map m = (W p) / h itself, so the projection gathers one array
    // (count form: it bins pt = wbar o p, which the previous direction kernel wrote)
    launch_bin(d, st, d->cf ? d->pt : p, nullptr, d->h, num, flags, true, d->cf);   // empty rows of num stay 0
    // 4 launches per iteration: the p.q / r.r finals and the stop test are folded into
    // the update and direction kernels (k_dot_final's summation order)
    const unsigned pg = launch_project(d, st, p, num, nullptr, q, d->part, flags);
    double *part_rr = d->part + (size_t)d->nb * kPartMax;
    COMAP_NB_SWITCH(d->nb,
                    k_cg_update_fused<NB><<<upd_grid(d->NO), 256, 0, st>>>(d->scal, d->part, (int)pg, x, r, p, q,
                                                                           d->NO, part_rr, flags);
                    k_cg_direction_fused<NB><<<grid_for(d->NO, kDirBlocks), 256, 0, st>>>(
                        d->scal, part_rr, (int)upd_grid(d->NO), p, r, d->NO, d->flags, kPartMax,
                        d->cf ? d->wbar : nullptr, d->cf ? d->pt : nullptr));
}

// graph replay pays when an iteration's kernels are shorter than enqueueing them
// (~20 us of host time for 4 launches): below ~300k entries (C4's 4-band iteration of
// 0.5 M entries already runs 34 us)
static bool cg_use_graph(const comap_destriper *d)
{
    if (d->opt.cg_graph >= 0) return d->opt.cg_graph == 1;
    return d->nnz + d->nnzp < 300000;
}

// The CG stream, event, stop flags and pinned read-back blocks, created on first use (the ground
// solve shares them and brings its own vectors).
int ds_cg_state(comap_destriper *d)
{
    comap_ctx *ctx = d->ctx;
    const size_t nb = (size_t)d->nb;
    if (!d->flags && dalloc(ctx, &d->flags, 2 + 2 * nb)) return -2;
    if (!d->flags_host) COMAP_CHECK(ctx, comap_pinned_alloc((void **)&d->flags_host, 4 * (2 + 2 * nb)));
    if (!d->thr_host) COMAP_CHECK(ctx, comap_pinned_alloc((void **)&d->thr_host, 8 * (1 + 4 * nb)));
    if (!d->cs) COMAP_CHECK(ctx, comap_stream_acquire(&d->cs));
    if (!d->ev) COMAP_CHECK(ctx, hipEventCreateWithFlags(&d->ev, hipEventDisableTiming));
    return 0;
}

bool ds_cg_use_graph(const comap_destriper *d) { return cg_use_graph(d); }

// CG vectors, state and (small problems) the kCgBatch-iteration graph, created on first use.
static int cg_setup(comap_destriper *d)
{
    if (d->cg && (d->batch || !cg_use_graph(d))) return 0;
    comap_ctx *ctx = d->ctx;
    const size_t nb = (size_t)d->nb;
    if (!d->cg && dalloc(ctx, &d->cg, (4 * (size_t)d->NO + (size_t)d->npix) * nb)) return -2;
    if (const int rc = ds_cg_state(d)) return rc;
    if (!cg_use_graph(d)) return 0;
    hipGraph_t g = nullptr;
    COMAP_CHECK(ctx, hipStreamBeginCapture(d->cs, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < kCgBatch; ++i) enqueue_iteration(d, d->cs);
    COMAP_CHECK(ctx, hipStreamEndCapture(d->cs, &g));
    const hipError_t e = hipGraphInstantiate(&d->batch, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    COMAP_CHECK(ctx, e);
    return 0;
}

// Single-rank destriper_iteration for every band: CG (one matvec per iteration) to
// threshold / niter, then the final maps (:419-451).  Iterations are queued kCgBatch
// at a time as one graph launch; the device-side stop flags make a band's iterations
// after its convergence no-ops, so its iterates and count equal a per-iteration loop's.
// md: the problem the final maps are binned from -- d itself, or a solve-mask view's parent (the full
// weights), on the same stream behind the CG with no host wait between.
static int solve_on(comap_destriper *d, comap_destriper *md, double threshold, int32_t niter, double *x, double *map,
                    double *naive, double *weight, double *hits, int32_t *iters_out)
{
    if (!d || !x || niter < 0) return -1;
    COMAP_DEVICE_GUARD(d->ctx);
    comap_ctx *ctx = d->ctx;
    int rc = cg_setup(d);
    if (rc) return rc;
    hipStream_t st = d->cs;
    const int nb = d->nb;
    const int64_t n = d->NO * nb, np = d->npix * nb;
    double *cx = d->cg, *r = cx + n, *p = r + n, *num = p + 2 * n;
    // inputs were produced on the caller's stream
    COMAP_CHECK(ctx, hipEventRecord(d->ev, ctx->stream));
    COMAP_CHECK(ctx, hipStreamWaitEvent(st, d->ev, 0));
    d->thr_host[0] = threshold;
    COMAP_CHECK(ctx, hipMemcpyAsync(d->scal + 4 * nb, d->thr_host, 8, hipMemcpyHostToDevice, st));
    COMAP_CHECK(ctx, hipMemsetAsync(cx, 0, 8 * n, st));
    COMAP_CHECK(ctx, hipMemsetAsync(num, 0, 8 * np, st));   // the CG bin writes only the non-empty rows
    COMAP_CHECK(ctx, hipMemsetAsync(d->flags, 0, 4 * (2 + 2 * nb), st));
    // b = op_Ax(tod, extend=False); r = p = b (x0 = 0); rr = rr0 = b.b
    launch_project(d, st, nullptr, d->nnum, d->h, r, nullptr, nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    COMAP_CHECK(ctx, hipMemcpyAsync(p, r, 8 * n, hipMemcpyDeviceToDevice, st));
    if (d->cf) {   // the first bin's input pt = wbar o p (later ones come from the direction kernel)
        COMAP_NB_SWITCH(nb, k_scale<NB><<<grid_for(d->NO), 256, 0, st>>>(d->wbar, p, d->NO, d->pt, nullptr));
        COMAP_LAUNCH_CHECK(ctx);
    }
    if ((rc = dot(d, st, r, r, d->scal, nullptr))) return rc;
    COMAP_CHECK(ctx, hipMemcpyAsync(d->scal + nb, d->scal, 8 * nb, hipMemcpyDeviceToDevice, st));
    COMAP_CHECK(ctx, hipMemcpyAsync(d->scal + 3 * nb, d->scal, 8 * nb, hipMemcpyDeviceToDevice, st));   // current rr
    for (int i = 0; i < 2 + 2 * nb; ++i) d->flags_host[i] = 0;
    // Batches of kCgBatch iterations between host checks; after the first, the next batch
    // is sized from each running band's convergence rate over the last batch (delta =
    // rr / rr0 falls geometrically), so a solve that needs 2 more iterations does not
    // enqueue 14 no-op ones (4 launches each).  The iterates are unchanged: every
    // kernel still stops on the device flags.
    double *hs = d->thr_host + 1;                       // rr0 [nb] | rr [nb] | pq [nb] | rr_new [nb]
    std::vector<double> prev_delta(nb, -1.0);
    int next = kCgBatch;
    for (int enq = 0; enq < niter;) {
        const int k = std::min(next, niter - enq);
        if (k == kCgBatch && d->batch) {
            COMAP_CHECK(ctx, hipGraphLaunch(d->batch, st));
        } else {
            for (int i = 0; i < k; ++i) enqueue_iteration(d, st);
            COMAP_LAUNCH_CHECK(ctx);
        }
        enq += k;
        COMAP_CHECK(ctx, hipMemcpyAsync(d->flags_host, d->flags, 4 * (2 + 2 * nb), hipMemcpyDeviceToHost, st));
        COMAP_CHECK(ctx, hipMemcpyAsync(hs, d->scal, 8 * 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
        COMAP_CHECK(ctx, hipStreamSynchronize(st));
        if (d->flags_host[0]) break;
        next = kCgBatch;
        if (threshold > 0) {
            int est = 0;
            for (int b = 0; b < nb; ++b) {
                if (d->flags_host[2 + b]) continue;
                const double delta = hs[3 * nb + b] / hs[b];
                const double pd = prev_delta[b] > 0 ? prev_delta[b] : 1.0;
                prev_delta[b] = delta;
                if (!(delta > 0) || !(delta < pd)) { est = kCgBatch; break; }
                const double need = std::log(threshold / delta) / (std::log(delta / pd) / k);
                est = std::max(est, (int)std::ceil(std::max(need, 0.0)) + 1);
            }
            next = std::max(1, std::min(kCgBatch, est));
        }
    }
    if (iters_out)
        for (int b = 0; b < nb; ++b) iters_out[b] = d->flags_host[2 + nb + b];
    COMAP_NB_SWITCH(nb, k_unpermute<NB><<<grid_for(d->NO), 256, 0, st>>>(cx, d->perm, d->NO, x));
    COMAP_LAUNCH_CHECK(ctx);
    // final maps: map = (sum w tod - W x) / h ; naive = sum w tod / h
    if (map) {
        launch_bin(md, st, cx, md->nnum, nullptr, num, nullptr);
        k_div_map<<<grid_for(np), 256, 0, st>>>(num, md->h, np, map);
    }
    if (naive) k_div_map<<<grid_for(np), 256, 0, st>>>(md->nnum, md->h, np, naive);
    COMAP_LAUNCH_CHECK(ctx);
    if (weight) COMAP_CHECK(ctx, hipMemcpyAsync(weight, md->h, 8 * np, hipMemcpyDeviceToDevice, st));
    if (hits) COMAP_CHECK(ctx, hipMemcpyAsync(hits, md->hits, 8 * np, hipMemcpyDeviceToDevice, st));
    COMAP_CHECK(ctx, hipStreamSynchronize(st));
    return 0;
}

extern "C" int comap_destripe_solve(comap_destriper *d, double threshold, int32_t niter, double *x, double *map,
                                    double *naive, double *weight, double *hits, int32_t *iters_out)
{
    return solve_on(d, d, threshold, niter, x, map, naive, weight, hits, iters_out);
}

// comap_destripe_solve's CG on a solve-mask view (the system of the masked weights), then the final
// maps from the view's parent with the CG's own x: every sample binned with its full weight.
extern "C" int comap_destripe_solve_view(comap_destriper *view, double threshold, int32_t niter, double *x, double *map,
                                         double *naive, double *weight, double *hits, int32_t *iters_out)
{
    if (!view) return -1;
    if (!view->parent) return comap_fail(view->ctx, -1, "comap_destripe_solve_view: not a solve-mask view");
    return solve_on(view, view->parent, threshold, niter, x, map, naive, weight, hits, iters_out);
}
