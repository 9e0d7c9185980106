// destriper_keys.hip -- comap_relabel_pixels, comap_relabel_pixels_tiled, comap_offset_centroid_keys
// and their kernels: they work on the callers' pixel id arrays, not on a comap_destriper.
#include "destriper_internal.h"

namespace {
__device__ __forceinline__ int32_t relabel_one(int32_t p32, const int32_t *__restrict__ lut, int64_t npix, int64_t nt)
{
    const int64_t p = p32;
    if (p >= npix || p < -npix) return (int32_t)nt;
    return p >= 0 ? lut[p] : (int32_t)((int64_t)lut[npix + p] - nt);
}

// The tiled layout's id of row-major pixel p (destriper.tiled_layout): T x T tiles in
// row-major tile order (ntx tiles a row), Morton order inside (bits of x at even, of y at
// odd positions) -- computed, not looked up: the table gathers ran at 1.9 TB/s on the field.
__device__ __forceinline__ int32_t tiled_id(int32_t p, int32_t nx, int32_t ntx, int tb, double inv)
{
    int32_t y = (int32_t)((double)p * inv);
    int32_t x = p - y * nx;
    if (x < 0) { --y; x += nx; }
    else if (x >= nx) { ++y; x -= nx; }
    const int32_t T = 1 << tb;
    const uint32_t ix = (uint32_t)(x & (T - 1)), iy = (uint32_t)(y & (T - 1));
    uint32_t z = 0;
    for (int b = 0; b < tb; ++b) z |= (((ix >> b) & 1u) << (2 * b)) | (((iy >> b) & 1u) << (2 * b + 1));
    return (((y >> tb) * ntx + (x >> tb)) << (2 * tb)) + (int32_t)z;
}

__device__ __forceinline__ int32_t relabel_tiled_one(int32_t p, int32_t npix, int32_t nx, int32_t ntx, int tb,
                                                     double inv, int32_t nt)
{
    if (p >= npix || p < -npix) return nt;
    return p >= 0 ? tiled_id(p, nx, ntx, tb, inv) : tiled_id(npix + p, nx, ntx, tb, inv) - nt;
}

__global__ void k_relabel_tiled(const int32_t *__restrict__ pix, int64_t n, int32_t npix, int32_t nx, int32_t ntx,
                                int tb, int32_t nt, int32_t *__restrict__ out)
{
    const double inv = 1.0 / (double)nx;
    const int64_t n4 = ((uintptr_t)pix % 16 == 0 && (uintptr_t)out % 16 == 0) ? n / 4 : 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < n4; i += stride) {
        const int4 v = reinterpret_cast<const int4 *>(pix)[i];
        int4 r;
        r.x = relabel_tiled_one(v.x, npix, nx, ntx, tb, inv, nt);
        r.y = relabel_tiled_one(v.y, npix, nx, ntx, tb, inv, nt);
        r.z = relabel_tiled_one(v.z, npix, nx, ntx, tb, inv, nt);
        r.w = relabel_tiled_one(v.w, npix, nx, ntx, tb, inv, nt);
        reinterpret_cast<int4 *>(out)[i] = r;
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) out[i] = relabel_tiled_one(pix[i], npix, nx, ntx, tb, inv, nt);
}

// four ids per thread (16-B loads and stores; torch's blocks are 256-B aligned), the tail
// one by one
__global__ void k_relabel_pixels(const int32_t *__restrict__ pix, int64_t n, const int32_t *__restrict__ lut,
                                 int64_t npix, int64_t nt, int32_t *__restrict__ out)
{
    const int64_t n4 = ((uintptr_t)pix % 16 == 0 && (uintptr_t)out % 16 == 0) ? n / 4 : 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < n4; i += stride) {
        const int4 v = reinterpret_cast<const int4 *>(pix)[i];
        int4 r;
        r.x = relabel_one(v.x, lut, npix, nt);
        r.y = relabel_one(v.y, lut, npix, nt);
        r.z = relabel_one(v.z, lut, npix, nt);
        r.w = relabel_one(v.w, lut, npix, nt);
        reinterpret_cast<int4 *>(out)[i] = r;
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) out[i] = relabel_one(pix[i], lut, npix, nt);
}
}  // namespace

// key[o] = lut[round(mean y) nx + round(mean x)] over offset o's on-map samples
// (0 <= p < nx ny, row-major ids), n_internal when it has none.  L > 64 (shorter offsets take
// the LDS kernel below): one wave per offset, a lane
// per sample (coalesced), 32-bit sums reduced across the wave; p = y nx + x by a double
// reciprocal and one integer fix-up (exact for p < 2^31).  (64-bit divisions and sums took
// 1.7 ms on the field's 4.38 M offsets, a thread per offset with strided loads as long,
// profiles/r06/r06c-d.)
__global__ void __launch_bounds__(256) k_offset_centroid_keys(const int32_t *__restrict__ pix, int64_t NO, int L,
                                                              int32_t nx, int32_t ny, const int32_t *__restrict__ lut,
                                                              int32_t n_internal, int32_t *__restrict__ key)
{
    const int lane = threadIdx.x & 63;
    const double inv = 1.0 / (double)nx;
    const int32_t npix = nx * ny;
    for (int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < NO; o += (int64_t)gridDim.x * 4) {
        int32_t sy = 0, sx = 0, c = 0;
        for (int j = lane; j < L; j += 64) {
            const int32_t p = pix[o * L + j];
            if (p >= 0 && p < npix) {
                int32_t y = (int32_t)((double)p * inv);
                int32_t x = p - y * nx;
                if (x < 0) { --y; x += nx; }
                else if (x >= nx) { ++y; x -= nx; }
                sy += y;
                sx += x;
                c += 1;
            }
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) {
            sy += __shfl_xor(sy, sh, 64);
            sx += __shfl_xor(sx, sh, 64);
            c += __shfl_xor(c, sh, 64);
        }
        if (lane == 0) {
            int32_t k = n_internal;
            if (c > 0) {
                const int32_t yi = (2 * sy + c) / (2 * c), xi = (2 * sx + c) / (2 * c);   // round half up
                k = lut[yi * nx + xi];
            }
            key[o] = k;
        }
    }
}

// The same keys for L <= 64, a block per 128 offsets: the block's 128 L pixel ids are one
// contiguous run, staged in LDS by coalesced loads (every load of the block in flight at
// once), then a thread per offset sums its samples from LDS -- one memory round trip per
// 128 offsets instead of one per offset (the wave-per-offset kernel above: 765 us on the
// field's 4.38 M offsets, latency-bound at 1.1 TB/s).
constexpr int kCkOffsets = 128;
__global__ void __launch_bounds__(256) k_offset_centroid_keys_lds(const int32_t *__restrict__ pix, int64_t NO, int L,
                                                                  int32_t nx, int32_t ny,
                                                                  const int32_t *__restrict__ lut, int32_t n_internal,
                                                                  int32_t *__restrict__ key)
{
    __shared__ int32_t sp[kCkOffsets * 64];
    const int64_t o0 = (int64_t)blockIdx.x * kCkOffsets;
    const int no = (int)min<int64_t>(kCkOffsets, NO - o0);
    const int cnt = no * L;
    const int32_t *src = pix + o0 * L;
    for (int i = threadIdx.x; i < cnt; i += 256) sp[i] = src[i];
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= no) return;
    const double inv = 1.0 / (double)nx;
    const int32_t npix = nx * ny;
    int32_t sy = 0, sx = 0, c = 0;
    for (int j = 0; j < L; ++j) {
        const int32_t p = sp[t * L + j];
        if (p >= 0 && p < npix) {
            int32_t y = (int32_t)((double)p * inv);
            int32_t x = p - y * nx;
            if (x < 0) { --y; x += nx; }
            else if (x >= nx) { ++y; x -= nx; }
            sy += y;
            sx += x;
            c += 1;
        }
    }
    int32_t k = n_internal;
    if (c > 0) {
        const int32_t yi = (2 * sy + c) / (2 * c), xi = (2 * sx + c) / (2 * c);   // round half up
        k = lut[yi * nx + xi];
    }
    key[o0 + t] = k;
}

extern "C" int comap_offset_centroid_keys(comap_ctx *ctx, const int32_t *pix, int64_t n, int32_t L, int64_t nx,
                                          int64_t ny, const int32_t *lut, int64_t n_internal, int32_t *key)
{
    if (!ctx || L < 1 || n < 0 || n % L || nx < 1 || ny < 1 || n_internal < nx * ny || n_internal >= (1ll << 31) ||
        (n > 0 && (!pix || !lut || !key)))
        return -1;
    COMAP_DEVICE_GUARD(ctx);
    const int64_t NO = n / L;
    if (NO == 0) return 0;
    if ((int64_t)L * (nx - 1 + ny - 1) >= (1ll << 30) / 2)     // the per-offset int32 sums
        return comap_fail(ctx, -1, "comap_offset_centroid_keys: map too large for the offset length");
    if (L <= 64 && (NO + kCkOffsets - 1) / kCkOffsets < (1ll << 31))
        k_offset_centroid_keys_lds<<<(unsigned)((NO + kCkOffsets - 1) / kCkOffsets), 256, 0, ctx->stream>>>(
            pix, NO, L, (int32_t)nx, (int32_t)ny, lut, (int32_t)n_internal, key);
    else
        k_offset_centroid_keys<<<(unsigned)std::min<int64_t>((NO + 3) / 4, 65536), 256, 0, ctx->stream>>>(
            pix, NO, L, (int32_t)nx, (int32_t)ny, lut, (int32_t)n_internal, key);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_relabel_pixels(comap_ctx *ctx, const int32_t *pix, int64_t n, const int32_t *lut, int64_t npix,
                                    int64_t n_internal, int32_t *out)
{
    if (!ctx || (n > 0 && (!pix || !lut || !out)) || n < 0 || npix <= 0 || n_internal < npix ||
        n_internal >= (1ll << 31))
        return -1;
    COMAP_DEVICE_GUARD(ctx);
    if (n == 0) return 0;
    k_relabel_pixels<<<grid_for((n + 3) / 4, 16384), 256, 0, ctx->stream>>>(pix, n, lut, npix, n_internal, out);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int comap_relabel_pixels_tiled(comap_ctx *ctx, const int32_t *pix, int64_t n, int64_t nx, int64_t ny,
                                          int32_t T, int32_t *out)
{
    if (!ctx || (n > 0 && (!pix || !out)) || n < 0 || nx < 1 || ny < 1 || T < 1 || (T & (T - 1)))
        return -1;
    int tb = 0;
    while ((1 << tb) < T) ++tb;
    const int64_t ntx = (nx + T - 1) / T, nty = (ny + T - 1) / T, nt = ntx * nty * T * T;
    if (nt >= (1ll << 31)) return -1;
    COMAP_DEVICE_GUARD(ctx);
    if (n == 0) return 0;
    k_relabel_tiled<<<grid_for((n + 3) / 4, 16384), 256, 0, ctx->stream>>>(pix, n, (int32_t)(nx * ny), (int32_t)nx,
                                                                           (int32_t)ntx, tb, (int32_t)nt, out);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}
