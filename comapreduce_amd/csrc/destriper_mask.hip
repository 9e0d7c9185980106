// destriper_mask.hip -- the solve mask's view of a destriper problem.
//
// A solve mask (MADAM's "inmask") fits the offsets from the samples outside a set of map pixels:
// w'_i = 0 where p_i >= 0 and mask[p_i], else w_i.  The CG then solves the reference system built
// from w', and everything after it -- the maps, the splits, the residuals -- uses the full w.
//
// The view is a second comap_destriper on the parent's index structure (orow, opix, prow, poff,
// sbase, spix, perm, hrow, hprow, wbar, hits, the launch shapes, the entry form), which it
// borrows, with its own
//   coefficients   ocnt / pcnt / sco (count form) or ow / pw / sco: the parent's, zero where the
//                  entry's pixel is masked.  Off-map entries (negative ids) keep theirs: their
//                  wrapped read m[npix + p] sees 0 on a masked pixel, as the reference's operator
//                  on w' does.  Sliced-ELLPACK padding slots stay padding.
//   ws' / tw'      the parent's values bit for bit on every offset that lost no entry; the others
//                  re-summed from their samples in a fixed order (lane order, then wave_sum).
//   h' / nnum'     the parent's maps with +0.0 on the masked pixels (every sample of a masked pixel
//                  is gone, so this is exact).
//   CG state       pt, part, scal and (on first use) the vectors, flags, stream, event and graph.
// Every existing entry point takes it as a comap_destriper.  comap_destripe_destroy frees only what
// the view owns; a parent with a live view is not destroyed.
#include "destriper_internal.h"

#include <memory>

namespace {

// the last row r with row[r] <= e (row[0] = 0 <= e < row[n])
__device__ __forceinline__ int64_t row_of(const int64_t *__restrict__ row, int64_t n, int64_t e)
{
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (row[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool masked_pixel(const uint8_t *__restrict__ mask, int32_t p, int64_t npix)
{
    return p >= 0 && p < npix && mask[p] != 0;
}

// CB bytes of entry e's coefficients, or zeros
template <int CB>
__device__ __forceinline__ void copy_coef(const void *__restrict__ src, void *__restrict__ dst, int64_t e, bool zero)
{
    if constexpr (CB % 8 == 0) {
        const double *s = reinterpret_cast<const double *>(src) + e * (CB / 8);
        double *d = reinterpret_cast<double *>(dst) + e * (CB / 8);
        double v[CB / 8];
        ldb<CB / 8>(s, v);
        if (zero) {
#pragma unroll
            for (int b = 0; b < CB / 8; ++b) v[b] = 0.0;
        }
        stb<CB / 8>(d, v);
    } else if constexpr (CB == 4) {
        reinterpret_cast<uint32_t *>(dst)[e] = zero ? 0u : reinterpret_cast<const uint32_t *>(src)[e];
    } else if constexpr (CB == 2) {
        reinterpret_cast<uint16_t *>(dst)[e] = zero ? (uint16_t)0 : reinterpret_cast<const uint16_t *>(src)[e];
    } else {
        reinterpret_cast<uint8_t *>(dst)[e] = zero ? (uint8_t)0 : reinterpret_cast<const uint8_t *>(src)[e];
    }
}

// Offset-major entries, a thread per entry (streaming): the coefficients copied or zeroed, and the
// offset of every zeroed entry flagged (its row by a search of orow: masked entries are few).
// Several entries of one offset store the same 1: no atomics.
template <int CB>
__global__ void __launch_bounds__(256) k_mask_offset_major(const int32_t *__restrict__ opix, const void *__restrict__ src,
                                                           const uint8_t *__restrict__ mask, int64_t nnz, int64_t npix,
                                                           const int64_t *__restrict__ orow, int64_t NO,
                                                           void *__restrict__ dst, int32_t *__restrict__ oflag)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x) {
        const bool z = masked_pixel(mask, opix[e], npix);
        copy_coef<CB>(src, dst, e, z);
        if (z) oflag[row_of(orow, NO, e)] = 1;
    }
}

// The sliced-ELLPACK copy, a thread per slot: padding slots (kSellPad) and off-map entries pass through.
template <int CB>
__global__ void __launch_bounds__(256) k_mask_sell(const int32_t *__restrict__ spix, const void *__restrict__ src,
                                                   const uint8_t *__restrict__ mask, int64_t nsell, int64_t npix,
                                                   void *__restrict__ dst)
{
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nsell; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t p = spix[e];
        copy_coef<CB>(src, dst, e, p != kSellPad && masked_pixel(mask, p, npix));
    }
}

// Pixel-major entries: `lanes` lanes per non-empty pixel row (hrow / hprow, the CG bin's row list:
// every entry lies in one of them), lane-strided, so consecutive lanes copy consecutive entries.
template <int CB>
__global__ void __launch_bounds__(256) k_mask_pixel_major(const int32_t *__restrict__ hrow,
                                                          const int64_t *__restrict__ hprow, int64_t nh,
                                                          const void *__restrict__ src, const uint8_t *__restrict__ mask,
                                                          int64_t npix, int lanes, void *__restrict__ dst)
{
    const int sub = threadIdx.x & (lanes - 1);
    const int64_t step = (int64_t)gridDim.x * blockDim.x / lanes;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / lanes; i < nh; i += step) {
        const bool z = masked_pixel(mask, hrow[i], npix);
        const int64_t e1 = hprow[i + 1];
        for (int64_t e = hprow[i] + sub; e < e1; e += lanes) copy_coef<CB>(src, dst, e, z);
    }
}

// ws' / tw', one wave per offset k (internal order; offset perm[k] of the caller's): an offset that
// lost no entry copies the parent's values; a flagged one sums w' and w' tod over its samples --
// lane l takes samples l, l + 64, ... in that order, then wave_sum's butterfly.  w, tod: [NB][N].
template <int NB>
__global__ void __launch_bounds__(256) k_mask_sums(const int32_t *__restrict__ oflag, const int32_t *__restrict__ perm,
                                                   const int32_t *__restrict__ pix, const double *__restrict__ tod,
                                                   const double *__restrict__ w, const uint8_t *__restrict__ mask,
                                                   int64_t N, int64_t NO, int L, int64_t npix,
                                                   const double *__restrict__ ws0, const double *__restrict__ tw0,
                                                   double *__restrict__ ws, double *__restrict__ tw)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < NO; k += (int64_t)gridDim.x * 4) {
        if (!oflag[k]) {
            if (lane < NB) ws[k * NB + lane] = ws0[k * NB + lane];
            else if (lane < 2 * NB) tw[k * NB + lane - NB] = tw0[k * NB + lane - NB];
            continue;
        }
        const int64_t base = (int64_t)perm[k] * L;
        double sw[NB], st[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) sw[b] = st[b] = 0.0;
        for (int j = lane; j < L; j += 64) {
            const bool z = masked_pixel(mask, pix[base + j], npix);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const double wv = z ? 0.0 : w[(int64_t)b * N + base + j];
                sw[b] += wv;
                st[b] = fma(wv, tod[(int64_t)b * N + base + j], st[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            sw[b] = wave_sum(sw[b]);
            st[b] = wave_sum(st[b]);
        }
        if (lane == 0) {
            stb<NB>(ws + k * NB, sw);
            stb<NB>(tw + k * NB, st);
        }
    }
}

// h' / nnum': the parent's maps, +0.0 on the masked pixels (all NB values)
template <int NB>
__global__ void __launch_bounds__(256) k_mask_maps(const double *__restrict__ h0, const double *__restrict__ n0,
                                                   const uint8_t *__restrict__ mask, int64_t npix,
                                                   double *__restrict__ h, double *__restrict__ nn)
{
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        double a[NB], c[NB];
        ldb<NB>(h0 + p * NB, a);
        ldb<NB>(n0 + p * NB, c);
        if (mask[p]) {
#pragma unroll
            for (int b = 0; b < NB; ++b) a[b] = c[b] = 0.0;
        }
        stb<NB>(h + p * NB, a);
        stb<NB>(nn + p * NB, c);
    }
}

// the three entry passes at CB coefficient bytes per entry
template <int CB>
void launch_entries(const comap_destriper *d, comap_destriper *v, const uint8_t *mask, int32_t *oflag, hipStream_t st)
{
    const void *osrc = d->cf ? (const void *)d->ocnt : (const void *)d->ow;
    const void *psrc = d->cf ? (const void *)d->pcnt : (const void *)d->pw;
    void *odst = d->cf ? (void *)v->ocnt : (void *)v->ow;
    void *pdst = d->cf ? (void *)v->pcnt : (void *)v->pw;
    k_mask_offset_major<CB><<<grid_for(d->nnz, 8192), 256, 0, st>>>(d->opix, osrc, mask, d->nnz, d->npix, d->orow, d->NO,
                                                                    odst, oflag);
    if (d->sell)
        k_mask_sell<CB><<<grid_for(d->nsell, 8192), 256, 0, st>>>(d->spix, d->sco, mask, d->nsell, d->npix, v->sco);
    if (d->nh > 0) {
        const int64_t mean = d->nnzp / d->nh;
        const int lanes = mean >= 48 ? 64 : (mean >= 12 ? 16 : 4);
        k_mask_pixel_major<CB><<<grid_for(d->nh * lanes, 8192), 256, 0, st>>>(d->hrow, d->hprow, d->nh, psrc, mask, d->npix,
                                                                              lanes, pdst);
    }
}

}  // namespace

extern "C" int comap_destripe_mask_view(comap_destriper *d, const int32_t *pix, const double *tod, const double *w,
                                        const uint8_t *mask, comap_destriper **out)
{
    if (!d || !out) return -1;
    comap_ctx *ctx = d->ctx;
    *out = nullptr;
    if (!pix || !tod || !w || !mask) return comap_fail(ctx, -1, "solve mask: null input");
    if (d->parent) return comap_fail(ctx, -1, "solve mask: a view of a view is not supported");
    COMAP_DEVICE_GUARD(ctx);
    hipStream_t st = ctx->stream;
    const int64_t NO = d->NO, npix = d->npix;
    const size_t nbz = (size_t)d->nb;
    // the parent's sizes, launch shapes, options and borrowed index arrays by value; then what the view owns
    auto *v = new comap_destriper(*d);
    v->parent = d;
    v->nviews = 0;
    v->ow = v->pw = v->ws = v->tw = v->pt = v->h = v->nnum = v->part = v->scal = v->cg = nullptr;
    v->ocnt = v->pcnt = nullptr;
    v->sco = nullptr;
    v->flags = nullptr;
    v->flags_host = nullptr;
    v->thr_host = nullptr;
    v->cs = nullptr;
    v->ev = nullptr;
    v->batch = nullptr;
    ++d->nviews;
    std::unique_ptr<comap_destriper, int (*)(comap_destriper *)> own(v, comap_destripe_destroy);
    int rc = 0;
    if (d->cf) {
        rc |= dalloc(ctx, &v->ocnt, d->nnz * nbz);
        rc |= dalloc(ctx, &v->pcnt, d->nnz * nbz);
        if (d->sell) rc |= dalloc(ctx, (uint8_t **)&v->sco, d->nsell * nbz);
    } else {
        rc |= dalloc(ctx, &v->ow, d->nnz * nbz);
        rc |= dalloc(ctx, &v->pw, d->nnz * nbz);
        if (d->sell) rc |= dalloc(ctx, (double **)&v->sco, d->nsell * nbz);
    }
    for (double **p : {&v->ws, &v->tw, &v->pt}) rc |= dalloc(ctx, p, NO * nbz);
    for (double **p : {&v->h, &v->nnum}) rc |= dalloc(ctx, p, npix * nbz);
    rc |= dalloc(ctx, &v->part, 2 * nbz * (size_t)kPartMax);
    rc |= dalloc(ctx, &v->scal, 4 * nbz + 4);
    if (rc) return -2;
    DevTemps tmp(st);
    int32_t *oflag = nullptr;
    COMAP_CHECK(ctx, tmp.alloc(&oflag, NO));
    COMAP_CHECK(ctx, hipMemsetAsync(oflag, 0, 4 * (size_t)NO, st));
    const int cb = d->cf ? d->nb : 8 * d->nb;
    switch (cb) {
    case 1: launch_entries<1>(d, v, mask, oflag, st); break;
    case 2: launch_entries<2>(d, v, mask, oflag, st); break;
    case 4: launch_entries<4>(d, v, mask, oflag, st); break;
    case 8: launch_entries<8>(d, v, mask, oflag, st); break;
    case 16: launch_entries<16>(d, v, mask, oflag, st); break;
    default: launch_entries<32>(d, v, mask, oflag, st);
    }
    COMAP_LAUNCH_CHECK(ctx);
    const unsigned wg = (unsigned)std::max<int64_t>(1, std::min<int64_t>((NO + 3) / 4, 65536));
    COMAP_NB_SWITCH(d->nb, k_mask_sums<NB><<<wg, 256, 0, st>>>(oflag, d->perm, pix, tod, w, mask, d->N, NO, d->L, npix,
                                                              d->ws, d->tw, v->ws, v->tw);
                    k_mask_maps<NB><<<grid_for(npix), 256, 0, st>>>(d->h, d->nnum, mask, npix, v->h, v->nnum));
    COMAP_LAUNCH_CHECK(ctx);
    // (tmp's destructor waits for the stream: the flags are read by then)
    own.release();
    *out = v;
    return 0;
}
