// destriper_resid.hip -- residual chi-squared of a solved destriper problem per offset and per
// group of offsets ((observation, feed) groups, or any labelling): how well tod - F x - P m matches
// the weights that were claimed.
//
// Sample t of offset o = t / L, band b, is COUNTED when pix[t] >= 0, w[b][t] > 0 and the band kept
// the offset (keep NULL or keep[b][o] != 0).  A counted sample's term is
//     r = (tod[b][t] - x[o][b]) - map[pix[t]][b]        term = (w[b][t] r) r
// every difference and product rounded to f64 on its own; an uncounted sample's term is +0.0.  A
// negative pixel id is never binned, so it has no map value of its own: the CG's wrap read
// m[npix + p] is deliberately not used here.  A non-finite tod of a counted sample makes its sums
// NaN (a non-finite weight is not > 0 or makes the term non-finite as well): nothing hides it.
//
// Sums run in the LANE-TREE ORDER, which is part of the interface (mapmaking/destriper.py's
// lane_tree_sum restates it in numpy).  For a sequence v[0 .. n):
//   1. lane l of 64 adds v[l], v[l + 64], v[l + 128], ... in that order, starting from +0.0;
//   2. for s = 32, 16, 8, 4, 2, 1: a[l] = a[l] + a[l ^ s];
//   3. the result is lane 0's.
// off_sum[o][b] is that sum of the L terms of offset o (v[j] = the term of sample o L + j),
// off_cnt[o][b] its number of counted samples; grp_sum[g][b] is that sum of off_sum[o][b] over the
// offsets with group[o] == g in increasing o, grp_cnt[g][b] the integer sum of their counts.  The
// order does not depend on the launch shape, there are no floating-point atomics: two calls give
// the same bytes.
//
// k_rs_offsets: one wave per offset at a time, lanes over consecutive samples, so tod, w and pix
// load coalesced (512, 512 and 256 B per wave-load), x[o][.] is wave-uniform and map[pix][.] is
// the only gather (8 NB contiguous bytes per lane, one 32-byte access for four bands); the bands
// loop inside the lane, so pix and the gather address are formed once.  With L <= 64 an offset is
// a single round of loads, so a wave keeps kRsU offsets' loads in flight before it reduces them
// one by one; a longer offset is walked kRsU rounds (256 samples) at a time.  The butterfly is
// wave_sum / wave_sum_scatter (all bands' sums in one reduce-scatter; the same tree: a + b == b +
// a bit for bit), the counts come from the wave's ballot.
// Group stage: the N / L offsets keyed by their group (label -1 behind the sentinel G), sorted and
// cut into segments (ds_sorted_segments, destriper_segments.hip), one wave per segment.
// It needs no comap_destriper: the inputs are the caller's arrays, x in the caller's order.
#include "destriper_internal.h"

// every product below is rounded before it is added (hipcc contracts a * b + c by default)
#pragma clang fp contract(off)

namespace {

constexpr int kRsU = 4;   // rounds of loads a wave issues before it adds them: offsets (L <= 64) or rounds of one

// One sample as a lane holds it between its loads and its use.  p < 0: not binned (or no sample).
template <int NB>
struct RsSample {
    int64_t p;
    double t[NB], w[NB], m[NB];
};

// Sample t (in: the lane has one).  A pixel id outside [-npix, npix) is flagged and read as
// unbinned: no load leaves the map.
template <int NB>
__device__ __forceinline__ void rs_load(RsSample<NB> &s, bool in, int64_t t, const int32_t *__restrict__ pix,
                                        const double *__restrict__ tod, const double *__restrict__ w,
                                        const double *__restrict__ map, int64_t N, int64_t npix,
                                        int32_t *__restrict__ flag)
{
    int64_t p = in ? (int64_t)pix[t] : -1;
    if (p >= npix || p < -npix) {
        flag[0] = 1;
        p = -1;
    }
    s.p = p;
    // (an unbinned lane reads pixel 0's values, in bounds and never used: no divergent gather)
    double mv[NB];
    ldb<NB>(map + (p >= 0 ? p : 0) * NB, mv);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        s.t[b] = in ? tod[(int64_t)b * N + t] : 0.0;
        s.w[b] = in ? w[(int64_t)b * N + t] : 0.0;
        s.m[b] = mv[b];
    }
}

// acc[b] += the sample's term in band b, cnt[b] += the wave's counted samples (wave-uniform)
template <int NB>
__device__ __forceinline__ void rs_add(const RsSample<NB> &s, const double (&xv)[NB], const bool (&kept)[NB],
                                       double (&acc)[NB], int (&cnt)[NB])
{
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const bool counted = s.p >= 0 && s.w[b] > 0.0 && kept[b];
        const double r = (s.t[b] - xv[b]) - s.m[b];
        const double term = (s.w[b] * r) * r;
        acc[b] += counted ? term : 0.0;
        cnt[b] += __popcll(__ballot(counted));
    }
}

// steps 2 and 3 of the lane-tree order for every band at once: band b's total in out on lane
// b (64 / NB) (and its 64 / NB - 1 neighbours)
template <int NB>
__device__ __forceinline__ double rs_tree(double (&acc)[NB], int lane)
{
    if constexpr (NB == 1) {
        return wave_sum(acc[0]);
    } else {
        wave_sum_scatter<NB>(acc, lane);
        return acc[0];
    }
}

template <int NB>
__device__ __forceinline__ void rs_store(double tot, const int (&cnt)[NB], int lane, int64_t o,
                                         double *__restrict__ off_sum, int32_t *__restrict__ off_cnt)
{
    constexpr int kStep = 64 / NB;
    if (lane % kStep == 0) off_sum[o * NB + lane / kStep] = tot;
    if (lane == 0) {                    // (wave-uniform values)
#pragma unroll
        for (int b = 0; b < NB; ++b) off_cnt[o * NB + b] = cnt[b];
    }
}

template <int NB>
__device__ __forceinline__ void rs_offset_consts(int64_t o, int64_t NO, const double *__restrict__ x,
                                                 const uint8_t *__restrict__ keep, double (&xv)[NB], bool (&kept)[NB])
{
    ldb<NB>(x + o * NB, xv);
#pragma unroll
    for (int b = 0; b < NB; ++b) kept[b] = keep ? keep[(int64_t)b * NO + o] != 0 : true;
}

template <int NB>
__global__ void __launch_bounds__(256) k_rs_offsets(const int32_t *__restrict__ pix, const double *__restrict__ tod,
                                                    const double *__restrict__ w, const uint8_t *__restrict__ keep,
                                                    const double *__restrict__ x, const double *__restrict__ map,
                                                    int64_t N, int64_t NO, int L, int64_t npix,
                                                    double *__restrict__ off_sum, int32_t *__restrict__ off_cnt,
                                                    int32_t *__restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const int64_t gw = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if (L <= 64) {
        // one round per offset: kRsU offsets' loads in flight, then each offset's own tree
        for (int64_t o0 = gw * kRsU; o0 < NO; o0 += nw * kRsU) {
            RsSample<NB> s[kRsU];
#pragma unroll
            for (int u = 0; u < kRsU; ++u) {
                const int64_t o = o0 + u;
                rs_load<NB>(s[u], o < NO && lane < L, o * L + lane, pix, tod, w, map, N, npix, flag);
            }
#pragma unroll
            for (int u = 0; u < kRsU; ++u) {
                const int64_t o = o0 + u;
                if (o >= NO) break;                       // wave-uniform
                double xv[NB], acc[NB];
                bool kept[NB];
                int cnt[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) { acc[b] = 0.0; cnt[b] = 0; }
                rs_offset_consts<NB>(o, NO, x, keep, xv, kept);
                rs_add<NB>(s[u], xv, kept, acc, cnt);
                const double tot = rs_tree<NB>(acc, lane);
                rs_store<NB>(tot, cnt, lane, o, off_sum, off_cnt);
            }
        }
    } else {
        for (int64_t o = gw; o < NO; o += nw) {
            double xv[NB], acc[NB];
            bool kept[NB];
            int cnt[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) { acc[b] = 0.0; cnt[b] = 0; }
            rs_offset_consts<NB>(o, NO, x, keep, xv, kept);
            for (int j0 = 0; j0 < L; j0 += 64 * kRsU) {
                RsSample<NB> s[kRsU];
#pragma unroll
                for (int u = 0; u < kRsU; ++u) {
                    const int j = j0 + 64 * u + lane;
                    rs_load<NB>(s[u], j < L, o * L + j, pix, tod, w, map, N, npix, flag);
                }
#pragma unroll
                for (int u = 0; u < kRsU; ++u) rs_add<NB>(s[u], xv, kept, acc, cnt);     // increasing j: the lane's order
            }
            const double tot = rs_tree<NB>(acc, lane);
            rs_store<NB>(tot, cnt, lane, o, off_sum, off_cnt);
        }
    }
}

// key[o] = the offset's group, or the sentinel G for label -1 (in no group).
// flag[1]: a label outside [-1, G).
__global__ void k_rs_keys(const int32_t *__restrict__ group, int64_t NO, int64_t G, uint32_t *__restrict__ key,
                          int32_t *__restrict__ flag)
{
    for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < NO; o += (int64_t)gridDim.x * blockDim.x) {
        int64_t g = group[o];
        if (g < -1 || g >= G) { flag[1] = 1; g = -1; }
        key[o] = g < 0 ? (uint32_t)G : (uint32_t)g;
    }
}

// One wave per segment e = the sorted offsets [estart[e], estart[e + 1]) of one group, in
// increasing offset (the sort is stable): the lane-tree sum of their off_sum per band, the
// integer sum of their counts.  The sentinel's segment is skipped.
template <int NB>
__global__ void __launch_bounds__(256) k_rs_groups(const uint32_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                   const int32_t *__restrict__ estart, int64_t ne, int64_t NO,
                                                   uint32_t sentinel, const double *__restrict__ off_sum,
                                                   const int32_t *__restrict__ off_cnt, double *__restrict__ grp_sum,
                                                   int64_t *__restrict__ grp_cnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t gw = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t e = gw; e < ne; e += nw) {
        const int64_t i0 = estart[e], i1 = e + 1 < ne ? (int64_t)estart[e + 1] : NO;
        const uint32_t g = skey[i0];
        if (g >= sentinel) continue;                          // wave-uniform
        double acc[NB];
        int64_t cnt[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) { acc[b] = 0.0; cnt[b] = 0; }
        for (int64_t i = i0 + lane; i < i1; i += 64) {
            const int64_t o = sval[i];
            double v[NB];
            ldb<NB>(off_sum + o * NB, v);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                acc[b] += v[b];
                cnt[b] += off_cnt[o * NB + b];
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const int64_t c = cnt[b];
                const int lo = __shfl_xor((int)(uint32_t)c, s, 64), hi = __shfl_xor((int)(c >> 32), s, 64);
                cnt[b] = c + (((int64_t)hi << 32) | (uint32_t)lo);
            }
        }
        const double tot = rs_tree<NB>(acc, lane);
        constexpr int kStep = 64 / NB;
        if (lane % kStep == 0) grp_sum[(int64_t)g * NB + lane / kStep] = tot;
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < NB; ++b) grp_cnt[(int64_t)g * NB + b] = cnt[b];
        }
    }
}

}  // namespace

extern "C" int comap_destripe_residuals(comap_ctx *ctx, const int32_t *pix, const double *tod, const double *w,
                                        const uint8_t *keep, const double *x, const double *map, const int32_t *group,
                                        int32_t n_groups, int64_t n_samples, int32_t offset_length, int64_t npix,
                                        int32_t n_bands, double *off_sum, int32_t *off_cnt, double *grp_sum,
                                        int64_t *grp_cnt)
{
    if (!ctx) return -1;
    if (!pix || !tod || !w || !x || !map || !off_sum || !off_cnt)
        return comap_fail(ctx, -1, "residuals: null input or output");
    const bool groups = group != nullptr && n_groups > 0;
    if ((group != nullptr) != (n_groups > 0) || n_groups < 0)
        return comap_fail(ctx, -1, "residuals: group labels and n_groups go together (NULL and 0: no group stage)");
    if (groups && (!grp_sum || !grp_cnt)) return comap_fail(ctx, -1, "residuals: null group output");
    if (n_bands != 1 && n_bands != 2 && n_bands != 4) return comap_fail(ctx, -1, "residuals: n_bands must be 1, 2 or 4");
    if (npix < 1 || npix >= (int64_t(1) << 31)) return comap_fail(ctx, -1, "residuals: npix must lie in [1, 2^31)");
    if (n_samples < 0 || n_samples >= (int64_t(1) << 31)) return comap_fail(ctx, -1, "residuals: n_samples must fit 31 bits");
    if (offset_length < 1 || n_samples % offset_length)
        return comap_fail(ctx, -1, "residuals: n_samples must be a multiple of offset_length");
    COMAP_DEVICE_GUARD(ctx);
    hipStream_t st = ctx->stream;
    const int64_t N = n_samples, G = n_groups, NO = N / offset_length;
    // every group no offset belongs to is 0 and 0
    if (groups) {
        COMAP_CHECK(ctx, hipMemsetAsync(grp_sum, 0, sizeof(double) * (size_t)G * (size_t)n_bands, st));
        COMAP_CHECK(ctx, hipMemsetAsync(grp_cnt, 0, sizeof(int64_t) * (size_t)G * (size_t)n_bands, st));
    }
    if (N == 0) return 0;

    DevTemps tmp(st, false);    // freed behind the stream's work: the read-back below is the only host wait
    int32_t *flag = nullptr;
    COMAP_CHECK(ctx, tmp.alloc(&flag, 2));
    COMAP_CHECK(ctx, hipMemsetAsync(flag, 0, 8, st));
    {
        // 4 waves per block; a wave takes kRsU offsets (L <= 64) or one per turn
        const int64_t turns = offset_length <= 64 ? (NO + kRsU - 1) / kRsU : NO;
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((turns + 3) / 4, 65536));
        COMAP_NB_SWITCH(n_bands, k_rs_offsets<NB><<<grid, 256, 0, st>>>(pix, tod, w, keep, x, map, N, NO, offset_length,
                                                                         npix, off_sum, off_cnt, flag));
        COMAP_LAUNCH_CHECK(ctx);
    }
    ds_segments<uint32_t> seg;
    if (groups) {
        uint32_t *key = nullptr;
        COMAP_CHECK(ctx, tmp.alloc(&key, NO));
        k_rs_keys<<<grid_for(NO, 65536), 256, 0, st>>>(group, NO, G, key, flag);
        COMAP_LAUNCH_CHECK(ctx);
        if (const int rc = ds_sorted_segments(ctx, tmp, key, NO, bits_for((uint64_t)G + 1), flag, &seg)) return rc;
    } else {
        // no group stage: the pixel flag alone, still one host wait
        int32_t hf[2] = {0, 0};
        COMAP_CHECK(ctx, hipMemcpyAsync(hf, flag, sizeof(hf), hipMemcpyDeviceToHost, st));
        COMAP_CHECK(ctx, hipStreamSynchronize(st));
        seg.flag[0] = hf[0];
    }
    if (seg.flag[0]) return comap_fail(ctx, -3, "pixel index out of range for the map (>= npix or < -npix)");
    if (seg.flag[1]) return comap_fail(ctx, -4, "residuals: group label out of range (valid: -1 .. n_groups - 1)");
    if (!groups) return 0;
    const int64_t ne = seg.ne;
    if (ne < 1 || ne > NO) return comap_fail(ctx, -2, "residuals: bad segment count");
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ne + 3) / 4, 65536));
    COMAP_NB_SWITCH(n_bands, k_rs_groups<NB><<<grid, 256, 0, st>>>(seg.skey, seg.sval, seg.estart, ne, NO, (uint32_t)G,
                                                                    off_sum, off_cnt, grp_sum, grp_cnt));
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}
