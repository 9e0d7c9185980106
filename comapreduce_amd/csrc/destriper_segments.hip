// destriper_segments.hip -- sorted segments: the idiom the ground set-up (destriper_ground.hip), the
// split maps (destriper_split.hip) and the residuals' group stage (destriper_resid.hip) sum by.
//
// The caller keys every element i in [0, n) (its own kernel: what a key means and which of the two
// flag words it raises differ).  ds_sorted_segments then runs ONE stable radix sort of (key, i) over
// the bits the caller's keys need, marks the heads of the runs of equal key (k_seg_heads), selects
// their positions (DeviceSelect::Flagged over an iota) and brings the number of segments and the two
// flag words back in one piece (k_seg_sizes, one copy, the call's ONE host wait).  Segment e is the
// sorted positions [estart[e], estart[e + 1]) (n behind the last), all of key skey[estart[e]].
//
// Determinism.  The sort is stable, so sval rises within a segment: a caller that walks its segment
// in sorted order adds in element order, whatever the launch shape.  Every fixed-order sum of the
// three callers rests on this one property.
#include "destriper_internal.h"

#include <hipcub/hipcub.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace {

template <typename Key>
__global__ void k_seg_heads(const Key *__restrict__ skey, int64_t n, uint8_t *__restrict__ head)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        head[i] = (i == 0 || skey[i] != skey[i - 1]) ? 1 : 0;
}

// the read-back in one piece: segments, flags
__global__ void k_seg_sizes(const int64_t *__restrict__ ne, const int32_t *__restrict__ flag, int64_t *__restrict__ out)
{
    if (threadIdx.x == 0) { out[0] = ne[0]; out[1] = flag[0]; out[2] = flag[1]; }
}

}  // namespace

template <typename Key>
int ds_sorted_segments(comap_ctx *ctx, DevTemps &tmp, const Key *key, int64_t n, int bits, const int32_t *flag,
                       ds_segments<Key> *out)
{
    hipStream_t st = tmp.st;
    uint8_t *head = nullptr;
    int64_t *cnt = nullptr;
    char *cub = nullptr;
    COMAP_CHECK(ctx, tmp.alloc(&out->skey, n));
    COMAP_CHECK(ctx, tmp.alloc(&out->sval, n));
    COMAP_CHECK(ctx, tmp.alloc(&out->estart, n));
    COMAP_CHECK(ctx, tmp.alloc(&head, n));
    COMAP_CHECK(ctx, tmp.alloc(&cnt, 4));
    rocprim::counting_iterator<int32_t> iota(0);    // the sort's values: element i carries i
    size_t tb = 0, b1 = 0;
    COMAP_CHECK(ctx, rocprim::radix_sort_pairs(nullptr, tb, key, out->skey, iota, out->sval, (size_t)n, 0u, (unsigned)bits, st));
    COMAP_CHECK(ctx, hipcub::DeviceSelect::Flagged(nullptr, b1, iota, head, out->estart, cnt, (int)n, st));
    tb = std::max(tb, b1);
    COMAP_CHECK(ctx, tmp.alloc(&cub, tb));

    b1 = tb;
    COMAP_CHECK(ctx, rocprim::radix_sort_pairs(cub, b1, key, out->skey, iota, out->sval, (size_t)n, 0u, (unsigned)bits, st));
    k_seg_heads<Key><<<grid_for(n, 65536), 256, 0, st>>>(out->skey, n, head);
    COMAP_LAUNCH_CHECK(ctx);
    b1 = tb;
    COMAP_CHECK(ctx, hipcub::DeviceSelect::Flagged(cub, b1, iota, head, out->estart, cnt, (int)n, st));
    k_seg_sizes<<<1, 64, 0, st>>>(cnt, flag, cnt + 1);
    COMAP_LAUNCH_CHECK(ctx);
    int64_t hw[3] = {0, 0, 0};
    COMAP_CHECK(ctx, hipMemcpyAsync(hw, cnt + 1, sizeof(hw), hipMemcpyDeviceToHost, st));
    COMAP_CHECK(ctx, hipStreamSynchronize(st));
    out->ne = hw[0];
    out->flag[0] = hw[1];
    out->flag[1] = hw[2];
    return 0;
}

template int ds_sorted_segments<uint32_t>(comap_ctx *, DevTemps &, const uint32_t *, int64_t, int, const int32_t *,
                                          ds_segments<uint32_t> *);
template int ds_sorted_segments<uint64_t>(comap_ctx *, DevTemps &, const uint64_t *, int64_t, int, const int32_t *,
                                          ds_segments<uint64_t> *);
