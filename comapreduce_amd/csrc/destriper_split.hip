// destriper_split.hip -- per-label split maps of a solved destriper problem: the reference's
// "Create individual feed maps too" block (MapMaking/Destriper.py:487-501), which bins tod - F x per
// feed, completed for any labelling of the offsets (feeds, observations, a caller's own).
//
// Every offset carries one label in [-1, G).  For label g, band b and pixel p the samples t with
// label[t / L] == g and pix[t] == p are visited in increasing t:
//     weight += w_t       naive += tod_t w_t       num += (tod_t - x_{t / L}) w_t       hits += 1
// (hits only where the band kept the offset), every difference, product and sum rounded to f64 on its
// own: binFuncs.binValues' order on the selected samples, so the sums equal the reference's bit for
// bit.  Negative pixel ids are never binned; label -1 leaves an offset out of every split.
//
// One pass for all labels: the samples are keyed with label npix + pixel (a sentinel behind every
// row for an unbinned sample), sorted and cut into segments of equal key over the bits G npix needs
// (ds_sorted_segments, destriper_segments.hip), and each (segment, band) pair is summed by one lane in
// sorted order -- which is sample order, the sort being stable -- and stored to its slot of the
// [G][npix][nb] outputs, zeroed beforehand.  No floating-point atomics: two calls agree bit for
// bit.  A long row is a serial chain by the definition of the order; a lane keeps kSplitU samples'
// loads in flight ahead of the chain, which it then adds in order, and a wave with few long rows
// sums each of them together: 64 samples loaded at once, added lane by lane (the same chain).
//
// It needs no comap_destriper: the inputs are the caller's arrays and x in the caller's order.
#include "destriper_internal.h"

// every product below is rounded before it is added (hipcc contracts a * b + c by default, and its
// __dmul_rn / __dadd_rn are plain operators that contract too)
#pragma clang fp contract(off)

namespace {

constexpr int kSplitU = 8;   // samples whose loads a summing lane issues before it adds them in order
constexpr int64_t kSplitLong = 512;   // a row from this many samples on is a long row
constexpr int kSplitWaveRows = 8;     // a wave sums its long rows together when it holds at most this many

// key[t] = label npix + pixel, or the sentinel G npix for a sample no split bins (negative pixel
// id, label -1).  flag[0]: a label outside [-1, G); flag[1]: a pixel id outside [-npix, npix).
__global__ void k_sp_keys(const int32_t *__restrict__ pix, const int32_t *__restrict__ label, int64_t N, int L,
                          int64_t npix, int64_t G, uint32_t *__restrict__ key, int32_t *__restrict__ flag)
{
    const uint32_t sentinel = (uint32_t)(G * npix);
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < N; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t g = label[t / L];
        if (g < -1 || g >= G) { flag[0] = 1; g = -1; }
        int64_t p = pix[t];
        if (p >= npix || p < -npix) { flag[1] = 1; p = -1; }
        key[t] = (g < 0 || p < 0) ? sentinel : (uint32_t)(g * npix + p);
    }
}

// One batch of a long row as a wave holds it: lane l has the row's sample i + l -- its weight, its
// two products (rounded, as the serial path rounds them) -- or zeros past the row's end; kept =
// the batch's samples in kept offsets.
struct SplitBatch {
    double wv, pn, pm;
    int kept;
};

template <int NB>
__device__ __forceinline__ SplitBatch split_load_batch(const int32_t *__restrict__ sval, int64_t i, int64_t i1, int lane,
                                                       int L, int b, const double *__restrict__ tb,
                                                       const double *__restrict__ wb, const uint8_t *__restrict__ kb,
                                                       const double *__restrict__ x)
{
    const bool in = i + lane < i1;
    const int64_t t = in ? (int64_t)sval[i + lane] : 0;
    const int64_t o = t / L;
    const double tv = in ? tb[t] : 0.0, wv = in ? wb[t] : 0.0, xv = in ? x[o * NB + b] : 0.0;
    const bool kv = in && (kb ? kb[o] != 0 : true);
    SplitBatch r;
    r.wv = wv;
    r.pn = tv * wv;
    r.pm = (tv - xv) * wv;
    r.kept = __popcll(__ballot(kv));
    return r;
}

// A long row [i0, i1) of band b summed by the whole wave (every lane calls it with the same
// arguments and gets the same sums): 64 samples are loaded at once, one per lane -- the loads and
// the products do not depend on the sums -- and added lane by lane, i.e. in sorted order, the
// next batch's loads in flight meanwhile.  A lane past the row's end adds +0.0, which changes no
// sum (a sum that starts at +0.0 never becomes -0.0).
template <int NB>
__device__ __forceinline__ void split_row_wave(const int32_t *__restrict__ sval, int64_t i0, int64_t i1, int lane, int L,
                                               int b, const double *__restrict__ tb, const double *__restrict__ wb,
                                               const uint8_t *__restrict__ kb, const double *__restrict__ x,
                                               double &am, double &an, double &aw, int64_t &nh)
{
    am = an = aw = 0.0;
    nh = 0;
    SplitBatch cur = split_load_batch<NB>(sval, i0, i1, lane, L, b, tb, wb, kb, x);
    for (int64_t i = i0; i < i1; i += 64) {
        SplitBatch nxt = {0.0, 0.0, 0.0, 0};
        if (i + 64 < i1) nxt = split_load_batch<NB>(sval, i + 64, i1, lane, L, b, tb, wb, kb, x);
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            aw += read_lane(cur.wv, j);
            an += read_lane(cur.pn, j);
            am += read_lane(cur.pm, j);
        }
        nh += cur.kept;
        cur = nxt;
    }
}

// Lane (e, b): segment e = the sorted samples [estart[e], estart[e + 1]) of one (label, pixel),
// band b.  The four sums in sorted (= sample) order, no contraction (the pragma above), stored to slot
// key nb + b.  The sentinel's segment is skipped.  A row of kSplitLong samples or more is summed by
// the lane's whole wave (split_row_wave) when at most kSplitWaveRows lanes of the wave hold one:
// a wave of long rows throughout is faster lane-parallel.  Either way the order of the adds, hence
// every bit of the sums, is the same.
template <int NB>
__global__ void __launch_bounds__(256) k_sp_sum(const uint32_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                const int32_t *__restrict__ estart, int64_t ne, int64_t N, int64_t NO,
                                                int L, uint32_t sentinel, const double *__restrict__ tod,
                                                const double *__restrict__ w, const uint8_t *__restrict__ keep,
                                                const double *__restrict__ x, double *__restrict__ num,
                                                double *__restrict__ nnum, double *__restrict__ wgt,
                                                double *__restrict__ hits)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = ne * NB, stride = (int64_t)gridDim.x * blockDim.x;
    // (the loop bound is the wave's: every lane stays in the loop for the wave-wide steps)
    for (int64_t base = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x - lane); base < total; base += stride) {
        const int64_t idx = base + lane;
        bool live = idx < total;
        const int64_t e = live ? idx / NB : 0;
        const int b = live ? (int)(idx % NB) : 0;
        int64_t i0 = 0, i1 = 0;
        uint32_t key = sentinel;
        if (live) {
            i0 = estart[e];
            i1 = e + 1 < ne ? (int64_t)estart[e + 1] : N;
            key = skey[i0];
            live = key < sentinel;
        }
        const bool lng = live && i1 - i0 >= kSplitLong;
        const uint64_t lmask = __ballot(lng);
        const bool by_wave = __popcll(lmask) <= kSplitWaveRows;
        const double *__restrict__ tb = tod + (int64_t)b * N;
        const double *__restrict__ wb = w + (int64_t)b * N;
        const uint8_t *__restrict__ kb = keep ? keep + (int64_t)b * NO : nullptr;
        double am = 0.0, an = 0.0, aw = 0.0;
        int64_t nh = 0;
        if (live && !(lng && by_wave)) {
            for (int64_t i = i0; i < i1; i += kSplitU) {
                int64_t t[kSplitU];
                double tv[kSplitU], wv[kSplitU], xv[kSplitU];
                int kv[kSplitU];
#pragma unroll
                for (int u = 0; u < kSplitU; ++u) t[u] = sval[i + u < i1 ? i + u : i1 - 1];
#pragma unroll
                for (int u = 0; u < kSplitU; ++u) {
                    const int64_t o = t[u] / L;
                    tv[u] = tb[t[u]];
                    wv[u] = wb[t[u]];
                    xv[u] = x[o * NB + b];
                    kv[u] = kb ? (kb[o] != 0) : 1;
                }
#pragma unroll
                for (int u = 0; u < kSplitU; ++u) {
                    if (i + u < i1) {
                        aw += wv[u];
                        an += tv[u] * wv[u];
                        am += (tv[u] - xv[u]) * wv[u];
                        nh += kv[u];
                    }
                }
            }
        }
        if (by_wave) {
            for (uint64_t m = lmask; m; m &= m - 1) {          // wave-uniform
                const int src = __ffsll((unsigned long long)m) - 1;
                const int64_t j0 = __shfl((int)i0, src, 64), j1 = __shfl((int)i1, src, 64);
                const int sb = __shfl(b, src, 64);
                const uint8_t *__restrict__ skb = keep ? keep + (int64_t)sb * NO : nullptr;
                double rm, rn, rw;
                int64_t rh;
                split_row_wave<NB>(sval, j0, j1, lane, L, sb, tod + (int64_t)sb * N, w + (int64_t)sb * N, skb, x, rm, rn,
                                   rw, rh);
                if (lane == src) { am = rm; an = rn; aw = rw; nh = rh; }
            }
        }
        if (live) {
            const int64_t q = (int64_t)key * NB + b;
            num[q] = am;
            nnum[q] = an;
            wgt[q] = aw;
            hits[q] = (double)nh;
        }
    }
}

// map = num / weight where weight != 0, else num; the same for naive (comap_destripe_div_map's rule)
__global__ void k_sp_div(const double *__restrict__ num, const double *__restrict__ nnum, const double *__restrict__ wgt,
                         int64_t n, double *__restrict__ map, double *__restrict__ naive)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double h = wgt[i], a = num[i], c = nnum[i];
        map[i] = h != 0.0 ? a / h : a;
        naive[i] = h != 0.0 ? c / h : c;
    }
}

}  // namespace

extern "C" int comap_destripe_split_maps(comap_ctx *ctx, const int32_t *pix, const double *tod, const double *w,
                                         const uint8_t *keep, const double *x, const int32_t *label, int32_t n_labels,
                                         int64_t n_samples, int32_t offset_length, int64_t npix, int32_t n_bands,
                                         double *num, double *nnum, double *wgt, double *hits)
{
    if (!ctx) return -1;
    if (!pix || !tod || !w || !x || !label || !num || !nnum || !wgt || !hits)
        return comap_fail(ctx, -1, "split maps: null input or output");
    if (n_bands != 1 && n_bands != 2 && n_bands != 4) return comap_fail(ctx, -1, "split maps: n_bands must be 1, 2 or 4");
    if (n_labels < 1 || npix < 1 || (uint64_t)n_labels * (uint64_t)npix >= (uint64_t(1) << 31))
        return comap_fail(ctx, -1, "split maps: n_labels x npix must lie in [1, 2^31)");
    if (n_samples < 0 || n_samples >= (int64_t(1) << 31)) return comap_fail(ctx, -1, "split maps: n_samples must fit 31 bits");
    if (offset_length < 1 || n_samples % offset_length)
        return comap_fail(ctx, -1, "split maps: n_samples must be a multiple of offset_length");
    COMAP_DEVICE_GUARD(ctx);
    hipStream_t st = ctx->stream;
    const int64_t N = n_samples, G = n_labels, NO = N / offset_length;
    const size_t out_bytes = sizeof(double) * (size_t)G * (size_t)npix * (size_t)n_bands;
    // every slot no segment reaches is zero
    COMAP_CHECK(ctx, hipMemsetAsync(num, 0, out_bytes, st));
    COMAP_CHECK(ctx, hipMemsetAsync(nnum, 0, out_bytes, st));
    COMAP_CHECK(ctx, hipMemsetAsync(wgt, 0, out_bytes, st));
    COMAP_CHECK(ctx, hipMemsetAsync(hits, 0, out_bytes, st));
    if (N == 0) return 0;

    DevTemps tmp(st, false);    // freed behind the stream's work: the helper's read-back is the only host wait
    uint32_t *key = nullptr;
    int32_t *flag = nullptr;
    COMAP_CHECK(ctx, tmp.alloc(&key, N));
    COMAP_CHECK(ctx, tmp.alloc(&flag, 2));
    const uint32_t sentinel = (uint32_t)(G * npix);
    COMAP_CHECK(ctx, hipMemsetAsync(flag, 0, 8, st));
    k_sp_keys<<<grid_for(N, 65536), 256, 0, st>>>(pix, label, N, offset_length, npix, G, key, flag);
    COMAP_LAUNCH_CHECK(ctx);
    ds_segments<uint32_t> seg;
    if (const int rc = ds_sorted_segments(ctx, tmp, key, N, bits_for((uint64_t)sentinel + 1), flag, &seg)) return rc;
    if (seg.flag[1]) return comap_fail(ctx, -3, "pixel index out of range for the map (>= npix or < -npix)");
    if (seg.flag[0]) return comap_fail(ctx, -4, "split maps: label out of range (valid: -1 .. n_labels - 1)");
    const int64_t ne = seg.ne;
    if (ne < 1 || ne > N) return comap_fail(ctx, -2, "split maps: bad segment count");

    COMAP_NB_SWITCH(n_bands, k_sp_sum<NB><<<grid_for(ne * NB, 65536), 256, 0, st>>>(
                                 seg.skey, seg.sval, seg.estart, ne, N, NO, offset_length, sentinel, tod, w, keep, x, num,
                                 nnum, wgt, hits));
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_destripe_split_div(comap_ctx *ctx, const double *num, const double *nnum, const double *wgt,
                                        int64_t n, double *map, double *naive)
{
    if (!ctx) return -1;
    if (!num || !nnum || !wgt || !map || !naive || n < 0) return comap_fail(ctx, -1, "split maps: null input or output");
    if (n == 0) return 0;
    COMAP_DEVICE_GUARD(ctx);
    k_sp_div<<<grid_for(n, 65536), 256, 0, ctx->stream>>>(num, nnum, wgt, n, map, naive);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}
