// destriper_setup.hip -- set-up of the destriper's constant operator: the kernels from the
// offset order keys to the sample-level maps' walks, their launchers, and
// comap_destripe_create* (phases: above comap_destripe_create_bands).  The only destriper unit
// that sorts and scans (hipcub / rocprim) or reads the COMAP_DS_* environment (read_options).
#include "destriper_internal.h"

#include <hipcub/hipcub.hpp>
#include <rocprim/device/device_radix_sort.hpp>

#include <memory>
#include <utility>

namespace {

// Inclusive prefix sum over the 64 lanes by DPP: row_shr 1 / 2 / 4 / 8 inside each 16-lane
// row (zeros shifted in), then row_bcast 15 / 31 carry the row totals into the later rows.
// Every lane must be active.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}

// ---------------------------------------------------------------- set-up (comap_destripe_create_bands)
// Processing order of the offsets.  In time order the offsets in flight at once
// cover the whole scan pattern, so the projection's map gathers (npix x 8 NB bytes,
// 7.4 MB for 4 bands at 480^2) miss the 4 MB XCD L2s.  Sorting offsets by the pixel
// of their first on-map sample makes concurrently processed offsets look at one band
// of map rows, and puts offsets that cross the same pixels next to each other in the
// CG vectors (the bin's x gathers).  Key: that pixel (npix when the offset is all
// off-map); a stable sort keeps time order among equal keys.
// (one wave per offset: its pixels by coalesced loads, the first on-map one by a ballot;
// a thread per offset walked an off-map offset's L pixels one dependent load at a time)
__global__ void __launch_bounds__(256) k_offset_keys(const int32_t *__restrict__ pix, int64_t NO, int L, int64_t npix,
                                                     int32_t *__restrict__ key, int32_t *__restrict__ val)
{
    const int lane = threadIdx.x & 63;
    for (int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < NO; o += (int64_t)gridDim.x * 4) {
        int32_t k = (int32_t)npix;
        if (!pix) {                 // keys given by the caller: the sort's values only
            if (lane == 0) val[o] = (int32_t)o;
            continue;
        }
        for (int j0 = 0; j0 < L; j0 += 64) {
            const int j = j0 + lane;
            const int32_t p = j < L ? pix[o * L + j] : -1;
            const unsigned long long v = __ballot(p >= 0);
            if (v) {
                k = __shfl(p, __ffsll((long long)v) - 1, 64);
                break;
            }
        }
        if (lane == 0) {
            key[o] = k;
            val[o] = (int32_t)o;
        }
    }
}

__global__ void k_iota32(int32_t *__restrict__ v, int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        v[i] = (int32_t)i;
}

// Member-mask walk: a kept entry's slot record, written by the count pass at slot
// k L + r (offset k's r-th entry) -- pixel, packed per-band non-zero counts, member mask
// (sample j of the offset = bit j) -- one 16-B-aligned gather for the sample walk
template <int K>
struct alignas(16) SlotRec {
    int32_t pix;
    uint32_t cnt;
    uint64_t mask[K];
};
static_assert(sizeof(SlotRec<1>) == 16 && sizeof(SlotRec<2>) == 32 && sizeof(SlotRec<4>) == 48, "SlotRec");

// Orders a wave's LDS writes before its later LDS reads by other lanes (and reads before
// later overwrites) where each wave owns its LDS region: one wave's LDS operations execute
// in issue order, so only the compiler must keep them in place.  A workgroup-scope fence
// would also wait for every global load and store the wave has in flight (s_waitcnt
// vmcnt(0)): the next chunk's prefetched loads and the previous chunk's stores.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Offset rows of the sparse operator, one wave per row k (offset o = perm[k]): lane l
// holds samples l, l + 64, ... (K per lane, L <= 64 K).  The distinct pixels of the
// offset are found in first-occurrence order by a leader loop (the first pending
// sample leads, one ballot per chunk collects every sample with its pixel), so the
// work is one short scalar loop per distinct pixel instead of an L x L compare.  The
// group's head lane then sums its samples' weights per band in sample order (the
// reference's binValues order within the offset; the offset's rows are L1-resident
// after the coalesced loads).  An entry is kept when any band's sum is non-zero.
// Both count passes: cnt[k] (kept entries), ws / tw (sum w, sum w tod per band: lane order,
// then a fixed butterfly), wbar and the count-form test, nonfin[1] for a pixel out of range.
//   CountWalk:    (member-mask walk) per sample (tod w) per band, sample-major in the internal
//                 offset order (payload [N][NB]); the row's kept entries as SlotRec records in
//                 slots [k L, k L + cnt[k]) of srec; the hits of the groups without an entry
//                 (hextra, over the offsets keep keeps); nonfin[0] for non-finite tod.
//   CountPayload: (sorted-sample walk) per sample the sort key of the sample-level maps
//                 (pixel, npix when not binned), its index, and the packed payload {w_b,
//                 tod_b w_b} [N][2 NB] (the product rounded, as binValues(weights = tod * w)
//                 rounds it).  The row's kept entries go to slots [k L, k L + cnt[k]) of eval
//                 (pixel) / eoff (packed uint8 counts), in entry order: the count form's fill is
//                 then a compaction (k_ds_compact_cf) instead of a second leader loop.
//   Fill:         (f64 form) the row's entries at orow[k]: pixel (-1 = off-map), weights, and
//                 the pixel-major transpose's key / entry id / row.
// w, tod: band-major [NB][N].  Arrays another mode owns are NULL.
enum class RowsMode { CountWalk, CountPayload, Fill };

template <int K, int NB, RowsMode MODE>
__global__ void __launch_bounds__(256) k_ds_rows(const int32_t *__restrict__ pix, const double *__restrict__ w,
                                                 const double *__restrict__ tod, int64_t N, int64_t NO, int L,
                                                 int64_t npix, const int32_t *__restrict__ perm,
                                                 int64_t *__restrict__ cnt, double *__restrict__ ws,
                                                 double *__restrict__ tw, double *__restrict__ payload,
                                                 int32_t *__restrict__ skey, int32_t *__restrict__ sval,
                                                 double *__restrict__ wbar, int32_t *__restrict__ nonuni,
                                                 const int64_t *__restrict__ orow, int32_t *__restrict__ opix,
                                                 double *__restrict__ ow, int32_t *__restrict__ ekey,
                                                 int32_t *__restrict__ eval, int32_t *__restrict__ eoff,
                                                 SlotRec<K> *__restrict__ srec, uint32_t *__restrict__ hextra,
                                                 const uint8_t *__restrict__ keep, int32_t *__restrict__ nonfin)
{
#pragma clang fp contract(off)
    constexpr bool FILL = MODE == RowsMode::Fill;
    const int lane = threadIdx.x & 63;
    constexpr int32_t kNone = INT32_MIN;    // lanes past the offset's end (real pixels are >= -1)
    // the offset's weights, staged in LDS: the group sums below read their members from
    // here instead of one dependent global load per member (the count pass took 3.2 ms at
    // C5 with 4 bands, 80 % of its wave cycles waiting)
    __shared__ double wsh[4][K * 64 * NB];
    double *wl = wsh[threadIdx.x >> 6];
    // waves walk offsets k, k + nw, ... (grid-stride; the launch covers every offset
    // once up to the launcher's cap -- a persistent grid that loaded the next offset during the current
    // one's leader loop took 100+ VGPRs, half the occupancy, and was no faster, r04z)
    const int64_t nw = (int64_t)gridDim.x * 4;
    int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    int32_t qn[K];
    double wn[K][NB], tn[K][NB];
    auto fetch = [&](int64_t kk) {
        const int64_t bs = (int64_t)perm[kk] * L;
#pragma unroll
        for (int m = 0; m < K; ++m) {
            const int j = lane + 64 * m;
            qn[m] = j < L ? pix[bs + j] : kNone;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                wn[m][b] = j < L ? w[(int64_t)b * N + bs + j] : 0.0;
                if constexpr (!FILL) tn[m][b] = j < L ? tod[(int64_t)b * N + bs + j] : 0.0;
            }
        }
    };
    for (; k < NO; k += nw) {
    fetch(k);
    const int64_t o = perm[k];
    const int64_t base = o * L;
    int32_t q[K];
    unsigned long long rem[K];
    double ti[K][NB];
#pragma unroll
    for (int m = 0; m < K; ++m) {
        q[m] = qn[m];
        rem[m] = __ballot(lane + 64 * m < L);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if constexpr (FILL) wl[(64 * m + lane) * NB + b] = wn[m][b];
            else ti[m][b] = tn[m][b];
        }
    }
    // (the fill pass reads group members' weights from LDS; the count pass stages them only
    // for an offset whose weights fail the count-form test, below)
    if constexpr (FILL) wave_lds_sync();
    // leader loop: head lanes and their members (per chunk of the leader)
    bool head[K];
    unsigned long long mem[K][K];
#pragma unroll
    for (int m = 0; m < K; ++m) {
        head[m] = false;
#pragma unroll
        for (int c = 0; c < K; ++c) mem[m][c] = 0ull;
    }
    if constexpr (K == 1) {
        // one sample per lane: the groups by an LDS hash table instead of the leader loop's
        // ~30 dependent readlane / ballot rounds per offset -- every lane inserts its pixel
        // (linear probing, compare-and-swap), the slot keeps the smallest lane (the first
        // occurrence: the group's head, as the leader loop picks it) and the OR of the
        // members' lane bits.  Same heads, same masks.
        constexpr int kSlots = 128;
        constexpr int32_t kEmpty = INT32_MIN + 1;
        __shared__ int32_t hkey[4][kSlots], hmin[4][kSlots];
        __shared__ unsigned long long hmsk[4][kSlots];
        int32_t *hk = hkey[threadIdx.x >> 6], *hm = hmin[threadIdx.x >> 6];
        unsigned long long *hb = hmsk[threadIdx.x >> 6];
#pragma unroll
        for (int z = lane; z < kSlots; z += 64) {
            hk[z] = kEmpty;
            hm[z] = 64;
            hb[z] = 0ull;
        }
        wave_lds_sync();
        const bool valid = lane < L;
        int slot = (int)(((uint32_t)q[0] * 2654435761u) >> 25);
        if (valid) {
            for (;;) {
                const int32_t old = atomicCAS(&hk[slot], kEmpty, q[0]);
                if (old == kEmpty || old == q[0]) break;
                slot = (slot + 1) & (kSlots - 1);
            }
            atomicMin(&hm[slot], lane);
            atomicOr(&hb[slot], 1ull << lane);
        }
        wave_lds_sync();
        head[0] = valid && hm[slot] == lane;
        mem[0][0] = head[0] ? hb[slot] : 0ull;
    } else {
#pragma unroll
    for (int m = 0; m < K; ++m) {
        while (rem[m]) {
            // the leader's pixel by v_readlane (rem is wave-uniform): no LDS round trip
            // (ds_bpermute) on this loop's dependent chain
            const int ld = __builtin_amdgcn_readfirstlane(__ffsll((long long)rem[m]) - 1);
            const int32_t pl = __builtin_amdgcn_readlane(q[m], ld);
            unsigned long long mm[K];
#pragma unroll
            for (int c = 0; c < K; ++c) {
                mm[c] = c < m ? 0ull : __ballot(q[c] == pl);
                rem[c] &= ~mm[c];
            }
            if (lane == ld) {
                head[m] = true;
#pragma unroll
                for (int c = 0; c < K; ++c) mem[m][c] = mm[c];
            }
        }
    }
    }   // K > 1: the leader loop
    // count pass: the count-form test first -- per band, every non-zero weight finite and
    // equal to the first one (ballot + readlane) -- with the non-zero masks
    double wi[K][NB], refb[NB];
    unsigned long long nzm[NB][K];
    bool uni = true;
    if constexpr (!FILL) {
#pragma unroll
        for (int m = 0; m < K; ++m)
#pragma unroll
            for (int b = 0; b < NB; ++b) wi[m][b] = wn[m][b];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            double ref = 0.0;
            bool found = false, bad = false;
#pragma unroll
            for (int m = 0; m < K; ++m) {
                nzm[b][m] = __ballot(wi[m][b] != 0.0);
                if (!found && nzm[b][m]) {
                    found = true;
                    ref = read_lane(wi[m][b], __ffsll((long long)nzm[b][m]) - 1);
                }
            }
#pragma unroll
            for (int m = 0; m < K; ++m) {
                const double v = wi[m][b];
                bad |= v != 0.0 && (!isfinite(v) || v != ref);
            }
            refb[b] = ref;
            uni &= __ballot(bad) == 0ull;
        }
        if (!uni) {      // wave-uniform: the group sums below read members' weights
#pragma unroll
            for (int m = 0; m < K; ++m)
#pragma unroll
                for (int b = 0; b < NB; ++b) wl[(64 * m + lane) * NB + b] = wi[m][b];
            wave_lds_sync();
        }
    }
    // per head: the group's in-order weight sums per band (and, for the count form, its
    // number of non-zero-weight samples).  A uniform offset in the count pass needs only
    // the counts (its group sums are count x weight: non-zero iff the count is), which are
    // popcounts of member mask & non-zero mask -- no per-member loop
    double gs[K][NB];
    int gc[K][NB];
    bool keepe[K];
#pragma unroll
    for (int m = 0; m < K; ++m) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            gs[m][b] = 0.0;
            gc[m][b] = 0;
        }
        if (!FILL && uni) {
            bool any = false;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                int n = 0;
#pragma unroll
                for (int c = 0; c < K; ++c) n += __popcll(mem[m][c] & nzm[b][c]);
                gc[m][b] = n;
                any |= n != 0;
            }
            keepe[m] = head[m] && any;
            continue;
        }
        if (head[m]) {
            // members in sample order, all bands per member (one NB-wide LDS read each);
            // every band's sum keeps the member order
#pragma unroll
            for (int c = 0; c < K; ++c)
                for (unsigned long long bits = mem[m][c]; bits; bits &= bits - 1) {
                    const double *src = wl + (64 * c + (__ffsll((long long)bits) - 1)) * NB;
                    double v[NB];
#pragma unroll
                    for (int b = 0; b < NB; ++b) v[b] = src[b];
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        gs[m][b] += v[b];
                        gc[m][b] += v[b] != 0.0;
                    }
                }
        }
        bool any = false;
#pragma unroll
        for (int b = 0; b < NB; ++b) any |= gs[m][b] != 0.0;
        keepe[m] = head[m] && any;
    }
    if constexpr (!FILL) {
        int64_t c0 = 0;
#pragma unroll
        for (int m = 0; m < K; ++m) c0 += __popcll(__ballot(keepe[m]));
        bool nf = false;
#pragma unroll
        for (int m = 0; m < K; ++m) {
            const int j = lane + 64 * m;
            if (j < L) {
                const int64_t i = base + j;
                if constexpr (MODE == RowsMode::CountWalk) {
                    // member-mask walk: (tod w) per band, sample-major (NB doubles a sample)
                    // in the internal offset order (slot k L + j), so the walk needs no perm
                    double pt[NB];
#pragma unroll
                    for (int b = 0; b < NB; ++b) pt[b] = ti[m][b] * wi[m][b];
                    stb<NB>(payload + (k * L + j) * NB, pt);
                } else {
                    double pl[2 * NB];
#pragma unroll
                    for (int b = 0; b < NB; ++b) { pl[b] = wi[m][b]; pl[NB + b] = ti[m][b] * wi[m][b]; }
                    stb<2 * NB>(payload + i * 2 * NB, pl);
                    skey[i] = (q[m] >= 0 && q[m] < npix) ? q[m] : (int32_t)npix;
                    sval[i] = (int32_t)i;
                }
#pragma unroll
                for (int b = 0; b < NB; ++b) nf |= !isfinite(ti[m][b]);
            }
        }
        // flags[1]: a pixel index >= npix or < -npix (the caller's error: numpy's m[pointing]
        // raises IndexError there; a negative id marks an unbinned sample that reads m[npix + p])
        bool ob = false;
#pragma unroll
        for (int m = 0; m < K; ++m) ob |= q[m] != kNone && (q[m] >= npix || q[m] < -npix);
        if (__ballot(ob) && lane == 0) nonfin[1] = 1;
        // member-mask walk (no payload): hits of the groups that hold no entry (every weight
        // zero) by integer adds -- order-free, exact -- and a flag for non-finite tod, which
        // such groups would carry into the naive numerator (the set-up then takes the
        // payload walk, which reproduces that)
        if constexpr (MODE == RowsMode::CountWalk) {
            if (__ballot(nf) && lane == 0) nonfin[0] = 1;
#pragma unroll
            for (int m = 0; m < K; ++m)
                if (head[m] && !keepe[m] && q[m] >= 0 && q[m] < npix) {
                    uint32_t cnt_m = 0;
#pragma unroll
                    for (int c = 0; c < K; ++c) cnt_m += (uint32_t)__popcll(mem[m][c]);
#pragma unroll
                    for (int b = 0; b < NB; ++b)
                        if (!keep || keep[(int64_t)b * NO + o]) atomicAdd(hextra + (int64_t)q[m] * NB + b, cnt_m);
                }
        }
        // per band: the offset's sums (lane order, then wave_sum_scatter's fixed butterfly) and
        // the count-form test's result (ballot + readlane above instead of two more 6-step
        // reductions per band: most of the count pass's LDS-pipe time was 4 x 4 bpermute
        // butterflies, r04w)
        if (!uni && lane == 0) nonuni[0] = 1;
        double red[2 * NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            double sw = 0.0, st = 0.0;
#pragma unroll
            for (int m = 0; m < K; ++m) {
                sw += wi[m][b];
                if (lane + 64 * m < L) st = fma(wi[m][b], ti[m][b], st);   // fused, as before the rewrite
            }
            red[2 * b] = sw;
            red[2 * b + 1] = st;
            if (lane == 0) wbar[k * NB + b] = refb[b];
        }
        wave_sum_scatter<2 * NB>(red, lane);
        if ((lane & (64 / (2 * NB) - 1)) == 0) {
            const int idx = lane / (64 / (2 * NB));           // value held: band idx / 2, sum idx % 2
            (idx & 1 ? tw : ws)[k * NB + (idx >> 1)] = red[0];
        }
        if (lane == 0) cnt[k] = c0;
        int64_t r0 = k * L;
#pragma unroll
        for (int m = 0; m < K; ++m) {
            const unsigned long long bm = __ballot(keepe[m]);
            if (keepe[m]) {
                const int64_t si = r0 + __popcll(bm & ((1ull << lane) - 1ull));
                uint32_t pk = 0;
#pragma unroll
                for (int b = 0; b < NB; ++b) pk |= (uint32_t)(gc[m][b] & 255) << (8 * b);
                if constexpr (MODE == RowsMode::CountWalk) {
                    SlotRec<K> rc;
                    rc.pix = q[m];
                    rc.cnt = pk;
#pragma unroll
                    for (int c = 0; c < K; ++c) rc.mask[c] = mem[m][c];
                    srec[si] = rc;
                } else {
                    eval[si] = q[m];
                    eoff[si] = (int32_t)pk;
                }
            }
            r0 += __popcll(bm);
        }
    } else {
        int64_t e = orow[k];
#pragma unroll
        for (int m = 0; m < K; ++m) {
            const unsigned long long bm = __ballot(keepe[m]);
            if (keepe[m]) {
                const int64_t ei = e + __popcll(bm & ((1ull << lane) - 1ull));
                opix[ei] = q[m];
                // (the count form's fill is k_ds_compact_cf over the count pass's slots)
#pragma unroll
                for (int b = 0; b < NB; ++b) ow[ei * NB + b] = gs[m][b];
                ekey[ei] = (q[m] >= 0 && q[m] < npix) ? q[m] : (int32_t)npix;
                eval[ei] = (int32_t)ei;
                eoff[ei] = (int32_t)k;
            }
            e += __popcll(bm);
        }
    }
    }   // offsets of this wave
}

// Count-form fill: row k's kept entries, left by the count pass in slots
// [k L, k L + cnt_k) (pixel, packed uint8 counts per band), copied to the CSR rows at
// orow[k] with the transpose's sort pairs (pixel key, offset << 32 | counts) -- the
// same entries, in the same order, as the leader-loop fill pass wrote (1.2 ms of the
// C5 4-band set-up, r03l).  One wave per row.
template <int NB>
__global__ void __launch_bounds__(256) k_ds_compact_cf(const int64_t *__restrict__ orow, int64_t NO, int L,
                                                       int64_t npix, const int32_t *__restrict__ spx,
                                                       const int32_t *__restrict__ spk, int32_t *__restrict__ opix,
                                                       uint8_t *__restrict__ ocnt, int32_t *__restrict__ ekey,
                                                       uint64_t *__restrict__ epay)
{
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= NO) return;
    const int64_t e0 = orow[k], c = orow[k + 1] - e0;
    for (int64_t r = lane; r < c; r += 64) {
        const int32_t q = spx[k * L + r];
        const uint32_t pk = (uint32_t)spk[k * L + r];
        const int64_t ei = e0 + r;
        opix[ei] = q;
        if constexpr (NB == 4) {
            *reinterpret_cast<uint32_t *>(ocnt + ei * 4) = pk;
        } else if constexpr (NB == 2) {
            *reinterpret_cast<uint16_t *>(ocnt + ei * 2) = (uint16_t)pk;
        } else {
            ocnt[ei] = (uint8_t)pk;
        }
        epay[ei] = ((uint64_t)(uint32_t)k << 32) | pk;
        ekey[ei] = (q >= 0 && q < npix) ? q : (int32_t)npix;
    }
}

// k_ds_rows' inputs, the same for its three modes (perm: the internal offset order)
struct RowsIn {
    const int32_t *pix;
    const double *w, *tod;
    int64_t N, NO, npix;
    int L, nb;
    const int32_t *perm;
};

// One wave per offset up to 2^20 blocks, grid-stride beyond (the field's 4.38 M offsets); callers
// use the three launchers below, which name what their mode reads and writes.
template <RowsMode MODE>
void launch_rows(const RowsIn &in, hipStream_t st, int64_t *cnt, double *ws, double *tw, double *payload, int32_t *skey,
                 int32_t *sval, double *wbar, int32_t *nonuni, const int64_t *orow, int32_t *opix, double *ow,
                 int32_t *ekey, int32_t *eval, int32_t *eoff, void *srec, uint32_t *hextra, const uint8_t *keep,
                 int32_t *flags)
{
    const unsigned blocks = (unsigned)std::min<int64_t>((in.NO + 3) / 4, 1 << 20);
#define COMAP_ROWS(K) k_ds_rows<K, NB, MODE><<<blocks, 256, 0, st>>>(in.pix, in.w, in.tod, in.N, in.NO, in.L, in.npix, \
                                                                     in.perm, cnt, ws, tw, payload, skey, sval, wbar, \
                                                                     nonuni, orow, opix, ow, ekey, eval, eoff, \
                                                                     (SlotRec<K> *)srec, hextra, keep, flags)
    COMAP_NB_SWITCH(in.nb, if (in.L <= 64) COMAP_ROWS(1);
                           else if (in.L <= 128) COMAP_ROWS(2);
                           else COMAP_ROWS(4));
#undef COMAP_ROWS
}

// count pass for the member-mask walk (ptw: (tod w) per sample [N][NB]; keep may be NULL;
// flags: [non-finite tod, pixel index out of range])
void rows_count_walk(const RowsIn &in, hipStream_t st, int64_t *cnt, double *ws, double *tw, double *wbar,
                     int32_t *nonuni, double *ptw, void *srec, uint32_t *hextra, const uint8_t *keep, int32_t *flags)
{
    launch_rows<RowsMode::CountWalk>(in, st, cnt, ws, tw, ptw, nullptr, nullptr, wbar, nonuni, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, srec, hextra, keep, flags);
}

// count pass for the sorted-sample walk (payload [N][2 NB] with its sort pairs skey / sval;
// spx / spk: the kept entries' pixel / packed counts by slot)
void rows_count_payload(const RowsIn &in, hipStream_t st, int64_t *cnt, double *ws, double *tw, double *wbar,
                        int32_t *nonuni, double *payload, int32_t *skey, int32_t *sval, int32_t *spx, int32_t *spk,
                        int32_t *flags)
{
    launch_rows<RowsMode::CountPayload>(in, st, cnt, ws, tw, payload, skey, sval, wbar, nonuni, nullptr, nullptr,
                                            nullptr, nullptr, spx, spk, nullptr, nullptr, nullptr, flags);
}

// f64 fill pass: the entries at orow, and the transpose's sort pairs (ekey, eid) and rows (eoff)
void rows_fill(const RowsIn &in, hipStream_t st, const int64_t *orow, int32_t *opix, double *ow, int32_t *ekey,
               int32_t *eid, int32_t *eoff)
{
    launch_rows<RowsMode::Fill>(in, st, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    orow, opix, ow, ekey, eid, eoff, nullptr, nullptr, nullptr, nullptr);
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

// Stable sort of int32 (key, value) pairs on key bits [0, end_bit): nine = rocprim's onesweep
// with 9-bit digits (match-based ranking: 512 buckets do not fit the basic rank's LDS) and
// no merge-sort path -- for the spatial offset sort, 18-bit pixel keys of 547 k offsets in
// 2 passes (63 us) instead of hipcub's ~20 block-merge kernels (131 us) at C5.  The
// transpose (15.4 M pairs) stays on hipcub's 8-bit onesweep: 410 us in 3 passes against
// 537 us in 2 with the match ranking (r04zr).  Keys are non-negative.
using Sort9Config = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 12>, rocprim::kernel_config<256, 12>, 9,
                                        rocprim::block_radix_rank_algorithm::match>,
    0>;

// (rocprim onesweep with 8-bit digits at 256 x 16 / 256 x 8 / 256 x 20 threads x items ran
// the transpose in 1.52 / 2.92 / 1.29 ms against hipcub's 0.43, r04ts: removed)
hipError_t sort_pairs_i32(bool nine, void *tmp, size_t &bytes, const int32_t *kin, int32_t *kout,
                          const int32_t *vin, int32_t *vout, int64_t n, int end_bit, hipStream_t st)
{
    if (nine)
        return rocprim::radix_sort_pairs<Sort9Config>(tmp, bytes, kin, kout, vin, vout, (unsigned)n, 0u,
                                                      (unsigned)end_bit, st);
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, kin, kout, vin, vout, (int)n, 0, end_bit, st);
}

// row[p] = first sorted position with key >= p, p in [0, npix]
__global__ void k_rowptr(const int32_t *__restrict__ skey, int64_t n, int64_t npix, int64_t *__restrict__ row)
{
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p <= npix; p += (int64_t)gridDim.x * blockDim.x)
        row[p] = lb32(skey, n, p);
}

// The set-up's first host read-back in one piece: nnz, the SELL slot count, the count-form
// and tod / pixel-range flags (four pageable copies cost ~20 us of idle GPU each)
__global__ void k_setup_sizes(const int64_t *__restrict__ orow, int64_t NO, const int64_t *__restrict__ sbase,
                              int64_t NCs, const int32_t *__restrict__ nonuni, const int32_t *__restrict__ flags,
                              int64_t *__restrict__ out)
{
    if (threadIdx.x == 0) {
        out[0] = orow[NO];
        out[1] = sbase ? sbase[NCs] : 0;
        out[2] = nonuni[0];
        out[3] = flags[0];
        out[4] = flags[1];
    }
}

// nat0[k] = orow_nat[perm[k]]: each internal row's first slot in the caller's-order entry
// array, gathered once so the compaction's rows need no dependent perm -> orow_nat load
__global__ void k_nat_base(const int64_t *__restrict__ orow_nat, const int32_t *__restrict__ perm, int64_t NO,
                           int64_t *__restrict__ nat0)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < NO; k += (int64_t)gridDim.x * blockDim.x)
        nat0[k] = orow_nat[perm[k]];
}

// cnt_nat[perm[k]] = cnt[k]: the offsets' kept-entry counts in the caller's offset order
__global__ void k_cnt_natural(const int64_t *__restrict__ cnt, const int32_t *__restrict__ perm, int64_t NO,
                              int64_t *__restrict__ cnt_nat)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k <= NO; k += (int64_t)gridDim.x * blockDim.x)
        cnt_nat[k < NO ? (int64_t)perm[k] : NO] = k < NO ? cnt[k] : 0;
}

// kint[k] = bit b set when band b keeps offset perm[k] (keep [nb][NO] in the caller's
// offset order): the sample walk reads one byte per entry by its internal offset k
__global__ void k_keep_bits(const uint8_t *__restrict__ keep, const int32_t *__restrict__ perm, int64_t NO, int nb,
                            uint8_t *__restrict__ kint)
{
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < NO; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = perm[k];
        uint32_t m = 0;
        for (int b = 0; b < nb; ++b) m |= (uint32_t)(keep[(int64_t)b * NO + o] != 0) << b;
        kint[k] = (uint8_t)m;
    }
}

// Count-form fill for the member-mask walk: row k's kept entries from the count pass's slots
// into the CSR rows (pixel, packed counts), and the transpose's sort pairs (pixel key, slot
// k L + r: the entry's walk record) in the caller's offset order (row k's first slot there:
// nat0[k], k_nat_base's gathered bases), so the stable sort by pixel leaves each pixel's entries in sample order -- the order binValues adds
// them in.  16 lanes per row (rows hold ~30 entries; a wave per row waited on its loads:
// 0.6 ms at C5).
template <int NB, int K>
__global__ void __launch_bounds__(256) k_ds_compact_walk(const int64_t *__restrict__ orow,
                                                         const int64_t *__restrict__ nat0, int64_t NO, int L,
                                                         int64_t npix, const SlotRec<K> *__restrict__ srec,
                                                         int32_t *__restrict__ opix, uint8_t *__restrict__ ocnt,
                                                         int32_t *__restrict__ ekey, int32_t *__restrict__ eval)
{
    const int sub = threadIdx.x & 15;
    const int64_t k = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (k >= NO) return;
    const int64_t e0 = orow[k], c = orow[k + 1] - e0, n0 = nat0[k];
    for (int64_t r = sub; r < c; r += 16) {
        const int32_t q = srec[k * L + r].pix;
        const uint32_t pk = srec[k * L + r].cnt;
        const int64_t ei = e0 + r;
        opix[ei] = q;
        if constexpr (NB == 4) {
            *reinterpret_cast<uint32_t *>(ocnt + ei * 4) = pk;
        } else if constexpr (NB == 2) {
            *reinterpret_cast<uint16_t *>(ocnt + ei * 2) = (uint16_t)pk;
        } else {
            ocnt[ei] = (uint8_t)pk;
        }
        ekey[n0 + r] = (q >= 0 && q < npix) ? q : (int32_t)npix;
        eval[n0 + r] = (int32_t)(k * L + r);
    }
}

// pixel-major entries (f64 form): sorted position k < nnzp (= prow[npix], read on the device) takes
// offset-major entry sval[k] (entries of one pixel come from spatially adjacent rows)
template <int NB>
__global__ void k_pixel_entries(const int32_t *__restrict__ sval, const int64_t *__restrict__ nnzp_dev,
                                const int32_t *__restrict__ eoff, const double *__restrict__ ow,
                                int32_t *__restrict__ poff, double *__restrict__ pw)
{
    const int64_t nnzp = *nnzp_dev;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < nnzp; k += (int64_t)gridDim.x * blockDim.x) {
        const int32_t e = sval[k];
        poff[k] = eoff[e];
        double v[NB];
        ldb<NB>(ow + (int64_t)e * NB, v);
        stb<NB>(pw + k * NB, v);
    }
}

// count form: pixel-major entries straight from the sorted (offset << 32 | counts) values
template <int NB>
__global__ void k_pixel_entries_cf(const uint64_t *__restrict__ pay, const int64_t *__restrict__ nnzp_dev,
                                   int32_t *__restrict__ poff, uint8_t *__restrict__ pcnt)
{
    const int64_t nnzp = *nnzp_dev;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < nnzp; k += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t v = pay[k];
        poff[k] = (int32_t)(v >> 32);
        const uint32_t c = (uint32_t)v;
        if constexpr (NB == 4) *reinterpret_cast<uint32_t *>(pcnt + k * 4) = c;
        else if constexpr (NB == 2) *reinterpret_cast<uint16_t *>(pcnt + k * 2) = (uint16_t)c;
        else pcnt[k] = (uint8_t)c;
    }
}

// Non-empty pixel rows for the CG bin: flag, exclusive scan, then the compact list with
// each row's entry range (hprow[i] = prow[hrow[i]], hprow[nh] = nnzp) and nh itself.
// h != NULL (member-mask walk, which visits the non-empty rows only): an empty row's
// sample-level maps here -- h = naive numerator = 0, hits = its zero-weight samples' count
__global__ void k_hit_flags(const int64_t *__restrict__ prow, int64_t npix, int32_t *__restrict__ flag, int nb,
                            const uint32_t *__restrict__ hextra, double *__restrict__ h, double *__restrict__ hits,
                            double *__restrict__ nnum, int64_t *__restrict__ counts)
{
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        const bool hit = prow[p + 1] > prow[p];
        flag[p] = hit ? 1 : 0;
        if (p == 0) counts[2] = 0;     // k_hit_rows' heavy-row count
        if (h && !hit)
            for (int b = 0; b < nb; ++b) {
                h[p * nb + b] = 0.0;
                nnum[p * nb + b] = 0.0;
                hits[p * nb + b] = (double)hextra[p * nb + b];
            }
    }
}

// heavy != NULL: also the list of the rows with more than heavy_min entries (any order,
// count in counts[2], which k_hit_flags zeroed) -- the sample walk starts them first
__global__ void k_hit_rows(const int64_t *__restrict__ prow, const int32_t *__restrict__ flag,
                           const int32_t *__restrict__ pos, int64_t npix, int32_t *__restrict__ hrow,
                           int64_t *__restrict__ hprow, int64_t *__restrict__ counts, int64_t heavy_min,
                           int32_t *__restrict__ heavy)
{
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        if (flag[p]) {
            hrow[pos[p]] = (int32_t)p;
            hprow[pos[p]] = prow[p];
            if (heavy && prow[p + 1] - prow[p] > heavy_min)
                heavy[atomicAdd(reinterpret_cast<unsigned long long *>(counts + 2), 1ull)] = pos[p];
        }
        if (p == npix - 1) {
            const int64_t nh = (int64_t)pos[p] + flag[p];
            hprow[nh] = prow[npix];
            counts[0] = prow[npix];   // nnzp
            counts[1] = nh;
        }
    }
}

// Sample-level maps in binValues order: h = sum w, hits = sum 1, nnum = sum tod w per
// pixel and band, over the samples of the offsets the band keeps (keep [NB][NO], NULL =
// all), each pixel's samples added one after the other in sample order (the stable
// pixel sort keeps it) -- the reference's sequential loop, bit for bit.
// One wave per pixel: per chunk of 64 of its samples every lane gathers one sample's
// packed payload (64 B for 4 bands) and keep mask into LDS, then lanes 0 .. 3 NB - 1
// each run one of the 3 NB ordered sums (h, nnum, hits per band) over the chunk.  The
// thread-per-pixel walk this replaces kept 8 gathers in flight per pixel, so the most
// hit pixel (thousands of samples) set the kernel time: 545 us on the chain's 3.4 M
// samples, 690 us at C5 (r03s2, r03l).
template <int NB>
__global__ void __launch_bounds__(256) k_sample_walk(const int64_t *__restrict__ srow, const int32_t *__restrict__ sval,
                                                     const double *__restrict__ payload, int64_t npix, int L, int64_t NO,
                                                     const uint8_t *__restrict__ keep, double *__restrict__ h,
                                                     double *__restrict__ hits, double *__restrict__ nnum)
{
    __shared__ double spl[4][64 * 2 * NB];
    __shared__ uint32_t smk[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *pl = spl[wv];
    uint32_t *mk = smk[wv];
    const int kind = lane / NB, b = lane % NB;     // this lane's ordered sum (lanes < 3 NB)
    const int col = kind == 2 ? 0 : kind * NB + b;
    for (int64_t p = (int64_t)blockIdx.x * 4 + wv; p < npix; p += (int64_t)gridDim.x * 4) {
        const int64_t lo = srow[p], hi = srow[p + 1];
        double acc = 0.0;
        for (int64_t c = lo; c < hi; c += 64) {
            const int n = (int)((hi - c) < 64 ? (hi - c) : 64);
            if (lane < n) {
                const int32_t i = sval[c + lane];
                double v[2 * NB];
                ldb<2 * NB>(payload + (int64_t)i * 2 * NB, v);
#pragma unroll
                for (int q = 0; q < 2 * NB; ++q) pl[lane * 2 * NB + q] = v[q];
                const int64_t o = i / L;
                uint32_t m = 0;
#pragma unroll
                for (int bb = 0; bb < NB; ++bb) m |= (uint32_t)(!keep || keep[(int64_t)bb * NO + o]) << bb;
                mk[lane] = m;
            }
            wave_lds_sync();   // the chunk, before other lanes read it
            if (lane < 3 * NB) {
                if (kind == 2) {
                    for (int t = 0; t < n; ++t) acc = ((mk[t] >> b) & 1u) ? acc + 1.0 : acc;
                } else {
#pragma unroll 8
                    for (int t = 0; t < n; ++t) {
                        const double v = pl[t * 2 * NB + col];
                        acc = ((mk[t] >> b) & 1u) ? acc + v : acc;
                    }
                }
            }
            wave_lds_sync();   // read before the next chunk overwrites
        }
        if (lane < 3 * NB) (kind == 0 ? h : kind == 1 ? nnum : hits)[p * NB + b] = acc;
    }
}

// every band's non-zero-weight count of a group is 0 or all n of its members (packed
// 8-bit counts): the group's weights are the offset's wb or zero
template <int NB>
__device__ __forceinline__ bool uniform_counts(uint32_t gc, uint32_t n)
{
    bool u = true;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint32_t c = (gc >> (8 * b)) & 255u;
        u = u && (c == 0u || c == n);
    }
    return u;
}

// position of the r-th (0-based) set bit of x (r < popcount(x)): six halving steps
__device__ __forceinline__ int select_bit(uint64_t x, int r)
{
    int pos = 0;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        const int c = __popcll(x & ((1ull << sh) - 1ull));
        if (r >= c) { r -= c; x >>= sh; pos += sh; }
    }
    return pos;
}

// Sample-level maps from the pixel-major entries (member-mask walk): one wave per pixel.
// Per chunk the wave takes the row's next entries (caller's offset order) whose members
// fit 64 M slots, one entry per lane (one packed-record gather each, which also writes the
// entry's pixel-major offset / counts for the CG bin); then every lane fills member slots
// t = lane + 64 u: the owning entry from the chunk's start-position mask, the member's
// sample from the entry's mask (sample order: an entry's members ascending, entries by
// offset), and its (w, tod w) per band into LDS.  tod w comes from the count pass's
// sample-major copy (ptw, one 8 NB-byte read); w is the offset's weight wb when all the
// group's members have a non-zero weight in the band (count form: they all equal wb), 0
// when none has, and only a mixed group reads w itself.  Then 2 NB lanes run the ordered
// sums of h and the naive numerator exactly as k_sample_walk does over the sorted samples.  Samples of groups without
// an entry carry zero weights (they add nothing to h or to the naive numerator); their
// hits come from the count pass's integer adds.
//
// The hits per band are integer counts (each kept member adds 1): they are summed as
// integers per entry instead of a third LDS column -- the same bits (exact below 2^53), a
// third less LDS per slot and 2 NB serial chains instead of 3 NB.
// heavy_min: entries above which a row is walked first (COMAP_DS_HEAVY, 0 = row order only).  Field walk
// (ms, r06w / r06x): 256: 9.00, 512: 8.20, 1024: 7.19, 1536: 6.89, 2048: 6.77-6.89, 3072: 7.00,
// 4096: 8.85 (15 rows), none: 9.45; C5 (max row 1047 entries) unaffected.
// The next chunk's records are prefetched one chunk ahead (field walk 7.23 vs 7.83 ms without,
// C5 1.17 vs 1.20 ms, r06m).  Its 73 VGPRs give 6 waves per SIMD; capped for 7: 7.28 ms, for 8: 9.05 ms
// with spills, r06n.  (The row list dealt to the XCDs in contiguous ranges: 8.23 vs 7.86 ms, r06l: removed.)
template <int NB, int K, int M>
__global__ void __launch_bounds__(256) k_sample_walk2(const int32_t *__restrict__ hrow,
                                                      const int64_t *__restrict__ hprow,
                                                      const int64_t *__restrict__ counts,
                                                      const int32_t *__restrict__ sval,
                                                      const SlotRec<K> *__restrict__ srec,
                                                      const int32_t *__restrict__ perm,
                                                      const double *__restrict__ wbar,
                                                      const double *__restrict__ w, const double *__restrict__ ptw,
                                                      int64_t N, int64_t npix, int L, int64_t NO,
                                                      const uint8_t *__restrict__ kint,
                                                      const uint32_t *__restrict__ hextra, double *__restrict__ h,
                                                      double *__restrict__ hits, double *__restrict__ nnum,
                                                      int32_t *__restrict__ poff, uint8_t *__restrict__ pcnt,
                                                      const int32_t *__restrict__ heavy, int64_t heavy_min)
{
#pragma clang fp contract(off)
    constexpr int CAP = 64 * M;
    // per member slot, 2 NB doubles: w and tod w per band, each 0 where the band does not
    // keep the member's offset -- adding +0 leaves a sum that never holds -0 unchanged, so
    // lane l < 2 NB runs its ordered sum as one unconditional chain over column l.  Slots are
    // SW doubles apart, SW odd: the 16 lanes of a ds_write_b64 group then hit distinct bank
    // pairs (an even stride would share bank pairs between lanes: multi-way conflicts)
    constexpr int SW = (2 * NB) | 1;
    __shared__ double spl[4][CAP * SW];
    __shared__ uint8_t sfl[4][CAP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *pl = spl[wv];
    uint8_t *fl = sfl[wv];
    const int kind = lane / NB, b = lane % NB;     // this lane's ordered sum (lanes < 2 NB)
    // the non-empty rows only (k_hit_flags wrote the empty ones): row i of nh = counts[1]
    // Each wave walks its heavy rows first (the long walks start at once, dealt round-robin
    // over the XCDs), then its rows of the row list.
    const int64_t nh = counts[1], nhv = heavy ? counts[2] : 0;
    const int64_t W = (int64_t)gridDim.x * 4, w0 = (int64_t)blockIdx.x * 4 + wv;
    // virtual rows: heavy v < nhv (this wave's w0, w0 + W, ...), then row v - nhv (w0, w0 + W, ...)
    auto next = [&](int64_t v) {
        if (v >= nhv) return v + W;
        v += W;
        return v < nhv ? v : nhv + w0;
    };
    for (int64_t ii = w0 < nhv ? w0 : nhv + w0; ii < nh + nhv; ii = next(ii)) {
        const int64_t i = ii < nhv ? (int64_t)heavy[ii] : ii - nhv;
        const int64_t lo = hprow[i], hi = hprow[i + 1];
        if (ii >= nhv && heavy && hi - lo > heavy_min) continue;     // walked from the heavy list
        const int64_t p = hrow[i];
        double acc = 0.0;
        uint32_t hc[NB];               // this lane's entries' kept members per band (hits)
#pragma unroll
        for (int q = 0; q < NB; ++q) hc[q] = 0;
        // slot ids of a chunk's entries: each chunk loads the next chunk's as soon as its own
        // extent is known (lanes past the row's end re-read its last entry: an unconditional
        // load, no select waiting on it).  The next chunk's records (member masks, counts,
        // keep bits) are gathered too, once those ids are in, while this chunk's member
        // gathers are in flight -- one dependent memory round trip per chunk instead of two
        // (every gather below is unconditional -- lanes past the chunk re-read valid entries --
        // so the compiler's wait for one load never has to drain the later ones: a load under
        // a branch makes it wait for all of them at the join)
        constexpr uint32_t kAll = (1u << NB) - 1u;
        const uint8_t *kip = kint ? kint : reinterpret_cast<const uint8_t *>(sval);
        int64_t si_c = sval[lo + lane < hi ? lo + lane : hi - 1];
        // the prefetched record as raw 16-B words (decoded at use: a SlotRec copy made the
        // compiler move the loaded registers at once, waiting for the load right there)
        constexpr int NQ = (int)(sizeof(SlotRec<K>) / 16);
        uint4 rq_n[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) rq_n[q] = reinterpret_cast<const uint4 *>(srec + si_c)[q];
        uint32_t kb_n = kip[si_c / L];
        for (int64_t c = lo; c < hi;) {
            const int64_t e = c + lane;
            const bool live = e < hi;
            // the entry's slot si = k L + r: its record from the count pass, the offset's
            // weights and keep bits from k
            const int64_t si = si_c;
            const int64_t kk = si / L;
            SlotRec<K> rc;
            double wb[NB];
            const uint32_t *wd = reinterpret_cast<const uint32_t *>(rq_n);
            rc.pix = (int32_t)wd[0];
            rc.cnt = wd[1];
#pragma unroll
            for (int q = 0; q < K; ++q) rc.mask[q] = (uint64_t)wd[2 + 2 * q] | ((uint64_t)wd[3 + 2 * q] << 32);
            const uint32_t kb = kint ? kb_n : kAll;
            ldb<NB>(wbar + kk * NB, wb);          // used after the member gathers are issued
            if (!live) {
                rc.pix = 0;
                rc.cnt = 0;
#pragma unroll
                for (int q = 0; q < K; ++q) rc.mask[q] = 0ull;
#pragma unroll
                for (int q = 0; q < NB; ++q) wb[q] = 0.0;
            }
            uint32_t cnt = 0;
#pragma unroll
            for (int q = 0; q < K; ++q) cnt += (uint32_t)__popcll(rc.mask[q]);
            // inclusive prefix of the member counts over the wave (DPP, no LDS permutes)
            const uint32_t inc = wave_incl_scan(cnt);
            const bool take = live && inc <= (uint32_t)CAP;
            const int ntake = __popcll(__ballot(take));     // >= 1: one entry holds <= L <= CAP members
            const int total = (int)__shfl(inc, ntake - 1, 64);
            const uint32_t excl = inc - cnt;
            if (take) {
#pragma unroll
                for (int q = 0; q < NB; ++q) hc[q] += ((kb >> q) & 1u) ? cnt : 0u;
                // the taken entries' pixel-major offset / counts for the CG bin
                poff[e] = (int32_t)kk;
                if constexpr (NB == 4) *reinterpret_cast<uint32_t *>(pcnt + e * 4) = rc.cnt;
                else if constexpr (NB == 2) *reinterpret_cast<uint16_t *>(pcnt + e * 2) = (uint16_t)rc.cnt;
                else pcnt[e] = (uint8_t)rc.cnt;
            }
            {
                const int64_t en = c + ntake + lane;
                si_c = sval[en < hi ? en : hi - 1];            // the next chunk's slot ids
            }
            // the chunk's entry start positions (taken entries hold >= 1 member each): each
            // taken entry flags its first slot in LDS, a ballot per 64 slots reads them back
            uint64_t sm[M];
#pragma unroll
            for (int u = 0; u < M; ++u) fl[lane + 64 * u] = 0;
            wave_lds_sync();
            if (take) fl[excl] = 1;
            wave_lds_sync();
#pragma unroll
            for (int u = 0; u < M; ++u) sm[u] = __ballot(fl[lane + 64 * u] != 0);
            // member slots t = lane + 64 u, first the owning entries and the member gathers ...
            int before = 0;                 // start positions in the slot words below u
            const uint64_t upto_lane = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
            int ju[M], bit[M];
            uint32_t nmu[M], ku[M], kbu[M], gcu[M];
            double pv[M][NB];
#pragma unroll
            for (int u = 0; u < M; ++u) {
                const int t = lane + 64 * u;
                // owning entry: start positions at or before t, minus one
                int j = before + __popcll(sm[u] & upto_lane);
                before += __popcll(sm[u]);
                j = t < total ? j - 1 : 0;
                ju[u] = j;
                const uint32_t exj = (uint32_t)__shfl((int)excl, j, 64);
                nmu[u] = (uint32_t)__shfl((int)cnt, j, 64);
                ku[u] = (uint32_t)__shfl((int)kk, j, 64);
                kbu[u] = (uint32_t)__shfl((int)kb, j, 64);
                gcu[u] = (uint32_t)__shfl((int)rc.cnt, j, 64);
                uint64_t mj[K];
#pragma unroll
                for (int q = 0; q < K; ++q) mj[q] = (uint64_t)__shfl((long long)rc.mask[q], j, 64);
                int r = t - (int)exj, bitpos = 0;
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const int cq = __popcll(mj[q]);
                    if (r >= 0 && r < cq) bitpos = 64 * q + select_bit(mj[q], r);
                    r -= cq;
                }
                bit[u] = bitpos;
                // (slots past the chunk: entry 0's first member, a valid address)
                ldb<NB>(ptw + ((int64_t)ku[u] * L + bitpos) * NB, pv[u]);
            }
            // a mixed group (some members zero-weight in a band): the sample's own weights
            double wmix[M][NB];
#pragma unroll
            for (int u = 0; u < M; ++u) {
                const int t = lane + 64 * u;
                if (t < total && !uniform_counts<NB>(gcu[u], nmu[u])) {
                    const int64_t on = perm[ku[u]];
#pragma unroll
                    for (int bb = 0; bb < NB; ++bb) {
                        const uint32_t gc = (gcu[u] >> (8 * bb)) & 255u;
                        wmix[u][bb] = gc != 0 && gc != nmu[u] ? w[(int64_t)bb * N + on * L + bit[u]] : 0.0;
                    }
                }
            }
            // ... then the next chunk's records (waits for its slot ids only) ...
#pragma unroll
            for (int q = 0; q < NQ; ++q) rq_n[q] = reinterpret_cast<const uint4 *>(srec + si_c)[q];
            kb_n = kip[si_c / L];
            // ... then the slots' (w, tod w) per band into LDS
#pragma unroll
            for (int u = 0; u < M; ++u) {
                const int t = lane + 64 * u;
                double wbj[NB];
#pragma unroll
                for (int q = 0; q < NB; ++q) wbj[q] = __shfl(wb[q], ju[u], 64);
                if (t < total) {
                    const uint32_t gcj = gcu[u], nmj = nmu[u];
                    double wvs[NB];
#pragma unroll
                    for (int bb = 0; bb < NB; ++bb) {
                        const uint32_t gc = (gcj >> (8 * bb)) & 255u;
                        wvs[bb] = gc == nmj ? wbj[bb] : 0.0;
                    }
                    if (!uniform_counts<NB>(gcj, nmj)) {
#pragma unroll
                        for (int bb = 0; bb < NB; ++bb) {
                            const uint32_t gc = (gcj >> (8 * bb)) & 255u;
                            if (gc != 0 && gc != nmj) wvs[bb] = wmix[u][bb];
                        }
                    }
#pragma unroll
                    for (int bb = 0; bb < NB; ++bb) {
                        const bool kept = (kbu[u] >> bb) & 1u;
                        pl[t * SW + bb] = kept ? wvs[bb] : 0.0;
                        pl[t * SW + NB + bb] = kept ? pv[u][bb] : 0.0;
                    }
                }
            }
            wave_lds_sync();   // the chunk, before other lanes read it
            if (lane < 2 * NB) {
#pragma unroll 8
                for (int t = 0; t < total; ++t) acc += pl[t * SW + lane];
            }
            wave_lds_sync();   // read before the next chunk overwrites
            c += ntake;
        }
        uint32_t hv = 0;               // lane q < NB: band q's hits over the row
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const uint32_t tq = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(hc[q]), 63);
            hv = lane == q ? tq : hv;
        }
        if (lane < 2 * NB) (kind == 0 ? h : nnum)[p * NB + b] = acc;
        if (lane < NB) hits[p * NB + lane] = (double)(hv + hextra[p * NB + lane]);
    }
}

// chunk widths: sw[c] = 64 x the longest row of offsets [64 c, 64 c + 64); sw[NC] = 0.
__global__ void k_sell_width(const int64_t *__restrict__ orow, int64_t NO, int64_t NC, int64_t *__restrict__ sw)
{
    const int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (c > NC) return;
    const int64_t o = c * 64 + (threadIdx.x & 63);
    int64_t len = (c < NC && o < NO) ? orow[o + 1] - orow[o] : 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) len = max(len, (int64_t)__shfl_xor(len, s, 64));
    if ((threadIdx.x & 63) == 0) sw[c] = 64 * len;
}

// The sliced-ELLPACK fill, one workgroup per chunk: the chunk's CSR range (contiguous: its offsets are
// consecutive rows) is staged in LDS with coalesced loads, then the padded column-major
// slots are written in order (coalesced, padding included: no memset).  Chunks holding more
// than kSellStage entries read their rows straight from global memory.
constexpr int kSellStage = 4096;
template <int NB, bool CF>
__global__ void __launch_bounds__(256) k_sell_fill_lds(const int64_t *__restrict__ orow,
                                                       const int32_t *__restrict__ opix,
                                                       const void *__restrict__ oco,
                                                       const int64_t *__restrict__ sbase, int64_t NO,
                                                       int32_t *__restrict__ spix, void *__restrict__ sco)
{
    // count form: an entry's NB uint8 counts moved as one NB-byte word (4 byte loads and
    // stores per entry were most of this kernel's instructions)
    using PackT = typename std::conditional<NB == 4, uint32_t, typename std::conditional<NB == 2, uint16_t, uint8_t>::type>::type;
    __shared__ int32_t lp[kSellStage];
    __shared__ PackT lc[CF ? kSellStage : 1];
    __shared__ int32_t rs[64], rn[64];
    constexpr int cw = 64;
    const int64_t c = blockIdx.x;
    const int64_t o0 = c * cw;
    const int nrow = (int)std::min<int64_t>(cw, NO - o0);
    const int64_t e0 = orow[o0];
    const int64_t ne = orow[o0 + nrow] - e0;
    if (threadIdx.x < cw) {
        const int r = threadIdx.x;
        rs[r] = r < nrow ? (int)(orow[o0 + r] - e0) : 0;
        rn[r] = r < nrow ? (int)(orow[o0 + r + 1] - orow[o0 + r]) : 0;
    }
    const bool staged = ne <= kSellStage && CF;
    if (staged) {
        for (int64_t i = threadIdx.x; i < ne; i += blockDim.x) {
            lp[i] = opix[e0 + i];
            lc[i] = reinterpret_cast<const PackT *>(oco)[e0 + i];
        }
    }
    __syncthreads();
    const int64_t b0 = sbase[c], nslot = sbase[c + 1] - b0;
    for (int64_t sl = threadIdx.x; sl < nslot; sl += blockDim.x) {
        const int r = (int)(sl % cw);
        const int64_t j = sl / cw;
        const bool in = j < rn[r];
        const int64_t ei = (int64_t)rs[r] + j;
        int32_t q = kSellPad;
        if constexpr (CF) {
            PackT a = 0;
            if (in) {
                q = staged ? lp[ei] : opix[e0 + ei];
                a = staged ? lc[ei] : reinterpret_cast<const PackT *>(oco)[e0 + ei];
            }
            spix[b0 + sl] = q;
            reinterpret_cast<PackT *>(sco)[b0 + sl] = a;
        } else {
            double a[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) a[k] = 0;
            if (in) {
                q = opix[e0 + ei];
#pragma unroll
                for (int k = 0; k < NB; ++k) a[k] = reinterpret_cast<const double *>(oco)[(e0 + ei) * NB + k];
            }
            spix[b0 + sl] = q;
#pragma unroll
            for (int k = 0; k < NB; ++k) reinterpret_cast<double *>(sco)[(b0 + sl) * NB + k] = a[k];
        }
    }
}

// One device allocation carved into the set-up's scratch arrays (256-B aligned): one hipMalloc /
// hipFree pair instead of one per array.  With a null base, take only advances `used`.
struct Arena {
    char *base = nullptr;
    size_t used = 0, cap = 0;
    hipStream_t st = nullptr;     // the set-up's stream: drained before the block goes back
    ~Arena()
    {
        (void)hipStreamSynchronize(st);
        if (base) comap_tmp_free_on((void *const *)&base, 1, st, true);
    }
    template <typename T>
    T *take(size_t n)
    {
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += (sizeof(T) * (n ? n : 1) + 255) & ~(size_t)255;
        return p;
    }
};

// What the phases of comap_destripe_create_keyed share; the scratch arrays are described in layout()
struct Setup {
    RowsIn in;                 // pix, w, tod, the sizes and the problem's perm
    const uint8_t *keep;       // [nb][NO] or NULL
    const int32_t *okey;       // the caller's offset order keys or NULL
    int end_bit = 1, key_bit = 1;   // radix bits of the pixel keys, of the offset order keys (the caller's bound or npix)
    int KW = 1;                // member-mask words per entry (k_ds_rows' K)
    size_t sort_tb = 0, sort64_tb = 0, scan_tb = 0, scan32_tb = 0, cub_tb = 0;   // hipcub temp storage
    int64_t NCs = 0;           // sliced-ELLPACK chunks
    int64_t *hw = nullptr;     // page-locked words of the two read-backs
    char *cub_tmp;
    int64_t *cnt, *srow, *counts, *swid, *cnt_nat, *orow_nat;
    int32_t *skey, *sval, *skey2, *sval2, *ekey, *eval, *ekey2, *eval2, *evn, *evn2, *eoff;
    int32_t *hflag, *hpos, *hheavy, *nonuni, *flags;
    double *payload;
    uint64_t *epay, *epay2;
    void *srec;
    uint32_t *hextra;
    uint8_t *kint;
};

// Sizes first (hipcub / rocprim temp storage for the largest sort / scan), then the arrays.
void layout(Arena &ar, Setup &s, const comap_destriper *d, hipStream_t st)
{
    const size_t N = (size_t)d->N, NO = (size_t)d->NO, npix = (size_t)d->npix, NB = (size_t)d->nb;
    (void)sort_pairs_i32(false, nullptr, s.sort_tb, nullptr, nullptr, nullptr, nullptr, N, s.end_bit, st);
    size_t tb9 = 0;       // the spatial offset sort (NO pairs)
    (void)sort_pairs_i32(true, nullptr, tb9, nullptr, nullptr, nullptr, nullptr, NO, s.key_bit, st);
    s.sort_tb = std::max(s.sort_tb, tb9);
    // the count form's transpose: (pixel, u64 offset|counts) pairs
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, s.sort64_tb, (int32_t *)nullptr, (int32_t *)nullptr,
                                             (uint64_t *)nullptr, (uint64_t *)nullptr, (int)N, 0, s.end_bit, st);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s.scan_tb, (int64_t *)nullptr, (int64_t *)nullptr, (int)(NO + 1), st);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s.scan32_tb, (int32_t *)nullptr, (int32_t *)nullptr, (int)npix, st);
    s.cub_tb = std::max({s.sort_tb, s.sort64_tb, s.scan_tb, s.scan32_tb});
    s.cub_tmp = ar.take<char>(s.cub_tb);
    s.cnt = ar.take<int64_t>(NO + 1);                                       // kept entries per row
    s.skey = ar.take<int32_t>(N), s.sval = ar.take<int32_t>(N);             // samples by pixel (sort in)
    s.skey2 = ar.take<int32_t>(N), s.sval2 = ar.take<int32_t>(N);           // (sort out)
    s.evn = s.skey2, s.evn2 = s.sval2;      // the walk's transpose values: the sample-sort arrays are free
    s.ekey = ar.take<int32_t>(N), s.eval = ar.take<int32_t>(N);             // entries by pixel (nnz <= N)
    s.ekey2 = ar.take<int32_t>(N), s.eval2 = ar.take<int32_t>(N);
    s.eoff = ar.take<int32_t>(N);
    s.payload = ar.take<double>(N * 2 * NB);
    s.srow = ar.take<int64_t>(npix + 1);
    s.hflag = ar.take<int32_t>(npix), s.hpos = ar.take<int32_t>(npix);
    s.hheavy = ar.take<int32_t>(npix);      // the walk's heavy rows (indices into hrow)
    s.counts = ar.take<int64_t>(8);         // [nnzp, nh, heavy rows] (k_hit_rows); first the set-up sizes (k_setup_sizes)
    s.nonuni = ar.take<int32_t>(1);
    s.epay = ar.take<uint64_t>(N), s.epay2 = ar.take<uint64_t>(N);          // count form: offset << 32 | counts
    s.swid = ar.take<int64_t>((NO + 31) / 32 + 1);      // sliced-ELLPACK chunk widths (64 offsets a chunk: ample)
    // member-mask walk (count form): slot / entry member masks, integer hits of the groups
    // without an entry, the transpose's rows in the caller's offset order
    s.srec = ar.take<uint64_t>(N * (s.KW == 1 ? 2 : s.KW == 2 ? 4 : 6));    // SlotRec<KW> per slot
    s.hextra = ar.take<uint32_t>(npix * NB);
    s.cnt_nat = ar.take<int64_t>(NO + 1), s.orow_nat = ar.take<int64_t>(NO + 1);
    s.flags = ar.take<int32_t>(2);          // [non-finite tod, pixel index out of range]
    s.kint = s.keep ? ar.take<uint8_t>(NO) : nullptr;   // keep bits by internal offset (sample walk)
}

int one_of(const char *v, int dflt, std::initializer_list<int> ok)
{
    const int x = v ? atoi(v) : dflt;
    for (int o : ok)
        if (x == o) return x;
    return dflt;
}

// The COMAP_DS_* options, read once per create (a variable set between two creates takes
// effect).  The launch shapes are measurement knobs: values outside their lists keep the defaults.
comap_ds_options read_options()
{
    comap_ds_options o;
    const char *v;
    if ((v = getenv("COMAP_DS_SELL"))) o.sell = v[0] == '1';
    if ((v = getenv("COMAP_DS_CF"))) o.cf = v[0] != '0';
    if ((v = getenv("COMAP_DS_WALK"))) o.walk = v[0] != '0';
    if ((v = getenv("COMAP_DS_HEAVY"))) o.heavy = atoll(v);
    o.bin_lanes = one_of(getenv("COMAP_DS_BL"), 0, {4, 8, 16, 32, 64});
    o.bin_u = one_of(getenv("COMAP_DS_BU"), 0, {4, 8});
    o.proj_lanes = one_of(getenv("COMAP_DS_PG"), 0, {4, 8, 16, 32, 64});
    o.proj_blocks = one_of(getenv("COMAP_DS_PB"), 0, {256, 512, 1024, 2048, 4096, 8192});
    o.cg_graph = one_of(getenv("COMAP_DS_CGGRAPH"), -1, {0, 1});
    return o;
}

// The count pass in the form the sample-level maps take.  Member-mask walk: no per-sample
// sort keys, but the slots' member masks, the empty groups' hits and the tod check.
// Payload walk: eval / eoff take the count-form fill's entry slots (unused by the f64 path
// until its own fill pass overwrites them).
void count_pass(comap_destriper *d, Setup &s, hipStream_t st)
{
    if (d->walk)
        rows_count_walk(s.in, st, s.cnt, d->ws, d->tw, d->wbar, s.nonuni, s.payload, s.srec, s.hextra, s.keep, s.flags);
    else
        rows_count_payload(s.in, st, s.cnt, d->ws, d->tw, d->wbar, s.nonuni, s.payload, s.skey, s.sval, s.eval, s.eoff,
                           s.flags);
}

}  // namespace

// ---- 1. spatial processing order of the offsets: by the caller's keys (comap_offset_centroid_keys:
// the centroid's internal pixel), or by the first on-map pixel of each offset
static int phase1_order(comap_destriper *d, Setup &s, hipStream_t st)
{
    comap_ctx *ctx = d->ctx;
    const int64_t NO = d->NO;
    if (s.okey)     // the sort's values only: a thread per offset
        k_iota32<<<grid_for(NO, 8192), 256, 0, st>>>(s.eval, NO);
    else
        k_offset_keys<<<(unsigned)std::min<int64_t>((NO + 3) / 4, 65536), 256, 0, st>>>(s.in.pix, NO, d->L, d->npix, s.ekey,
                                                                                         s.eval);
    COMAP_LAUNCH_CHECK(ctx);
    size_t tb = s.cub_tb;
    // (the caller's keys may exceed npix -- a compacted problem keeps its tiled-layout
    // keys -- so they sort on the bits of the caller's bound)
    COMAP_CHECK(ctx, sort_pairs_i32(true, s.cub_tmp, tb, s.okey ? s.okey : s.ekey, s.ekey2, s.eval, d->perm, NO,
                                    s.key_bit, st));
    return 0;
}

// ---- 2. count pass (+ the count-form test: non-zero weights uniform per offset and band),
// row pointers, the sliced-ELLPACK chunk bases
static int phase2_count(comap_destriper *d, Setup &s, hipStream_t st)
{
    comap_ctx *ctx = d->ctx;
    const int64_t NO = d->NO;
    COMAP_CHECK(ctx, hipMemsetAsync(s.nonuni, 0, 4, st));
    COMAP_CHECK(ctx, hipMemsetAsync(s.flags, 0, 8, st));
    if (d->walk) COMAP_CHECK(ctx, hipMemsetAsync(s.hextra, 0, 4 * (size_t)d->npix * d->nb, st));
    count_pass(d, s, st);
    COMAP_LAUNCH_CHECK(ctx);
    COMAP_CHECK(ctx, hipMemsetAsync(s.cnt + NO, 0, 8, st));
    COMAP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(s.cub_tmp, s.scan_tb, s.cnt, d->orow, (int)(NO + 1), st));
    if (d->walk) {
        k_cnt_natural<<<grid_for(NO + 1, 8192), 256, 0, st>>>(s.cnt, d->perm, NO, s.cnt_nat);
        COMAP_LAUNCH_CHECK(ctx);
        COMAP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(s.cub_tmp, s.scan_tb, s.cnt_nat, s.orow_nat, (int)(NO + 1), st));
        k_nat_base<<<grid_for(NO, 8192), 256, 0, st>>>(s.orow_nat, d->perm, NO, s.cnt_nat);   // (cnt_nat is free)
        COMAP_LAUNCH_CHECK(ctx);
    }
    // sliced-ELLPACK projection: default for large problems (C5, 547k offsets: 1 band
    // 0.112 -> 0.098 ms per CG iteration, 4 bands 0.261 -> 0.236, r04j); a C4-size problem
    // (35k offsets) gains nothing its extra set-up pass would not cost.  COMAP_DS_SELL=0/1
    d->sell = d->opt.sell >= 0 ? d->opt.sell == 1 : NO >= kSellMinOffsets;
    if (d->sell) {
        s.NCs = (NO + 63) / 64;
        if (dalloc(ctx, &d->sbase, s.NCs + 1)) return -2;
        const unsigned wg = (unsigned)(((s.NCs + 1) * 64 + 255) / 256);
        k_sell_width<<<wg, 256, 0, st>>>(d->orow, NO, s.NCs, s.swid);
        COMAP_LAUNCH_CHECK(ctx);
        COMAP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(s.cub_tmp, s.scan_tb, s.swid, d->sbase, (int)(s.NCs + 1), st));
    }
    return 0;
}

// Read-back 1 (sync 1): nnz, the SELL slot count and the count pass's flags in one piece;
// then what they decide -- entry form, launch shapes, the walk's fallback, the entry arrays
static int read_back_sizes(comap_destriper *d, Setup &s, hipStream_t st)
{
    comap_ctx *ctx = d->ctx;
    const int64_t NO = d->NO;
    const size_t NB = (size_t)d->nb;
    k_setup_sizes<<<1, 64, 0, st>>>(d->orow, NO, d->sell ? d->sbase : nullptr, s.NCs, s.nonuni, s.flags, s.counts);
    COMAP_LAUNCH_CHECK(ctx);
    COMAP_CHECK(ctx, hipMemcpyAsync(s.hw, s.counts, 5 * 8, hipMemcpyDeviceToHost, st));
    COMAP_CHECK(ctx, hipStreamSynchronize(st));
    d->nnz = s.hw[0];
    if (d->sell) d->nsell = s.hw[1];
    const bool nonfin = s.hw[3] != 0;
    if (s.hw[4]) return comap_fail(ctx, -3, "pixel index out of range for the map (>= npix or < -npix)");
    d->cf = !s.hw[2] && d->L <= 255 && d->opt.cf;
    // long pixel rows (the field: 376 entries per pixel) keep 8 entry loads in flight per
    // bin lane, and a problem of millions of offsets runs its SELL projection at 8192
    // blocks (field 4 bands: 1.446 -> 1.380 ms per iteration; C5 1 / 4 bands unchanged,
    // profiles/r06/r06cg).  Neither changes a result: a bin lane adds its entries in the
    // same order, and single-rank p.q partials are re-summed in one fixed order.
    const bool long_rows = d->nnz >= 256 * d->npix;
    d->bin_u = d->opt.bin_u ? d->opt.bin_u : (long_rows ? 8 : 4);
    // the SELL projection runs one chunk per wave at 2048 blocks (1024: 0.254 vs 0.244 ms per
    // 4-band C5 iteration, r04h); its p.q partials fit kPartMax and the dist slots
    d->proj_blocks = d->opt.proj_blocks ? d->opt.proj_blocks
                                        : (d->sell ? (NO >= (2 << 20) ? 8192 : 2 * kProjBlocks) : kProjBlocks);
    // the member-mask walk needs the count form and finite tod everywhere; otherwise the
    // count pass runs again with the per-sample payload for the sorted-sample walk
    if (d->walk && (!d->cf || nonfin)) {
        d->walk = false;
        count_pass(d, s, st);
        COMAP_LAUNCH_CHECK(ctx);
    }
    int rc = 0;
    rc |= dalloc(ctx, &d->opix, d->nnz);
    rc |= dalloc(ctx, &d->poff, d->nnz);          // nnzp <= nnz (off-map entries are not binned)
    if (d->cf) {
        rc |= dalloc(ctx, &d->ocnt, d->nnz * NB);
        rc |= dalloc(ctx, &d->pcnt, d->nnz * NB);
    } else {
        rc |= dalloc(ctx, &d->ow, d->nnz * NB);
        rc |= dalloc(ctx, &d->pw, d->nnz * NB);
    }
    return rc ? -2 : 0;
}

// ---- 3. fill pass: the offset-major entries, the transpose's sort pairs, the SELL copy
static int phase3_fill(comap_destriper *d, Setup &s, hipStream_t st)
{
    comap_ctx *ctx = d->ctx;
    const int64_t NO = d->NO, npix = d->npix;
    const int L = d->L, nb = d->nb;
    if (d->walk) {
#define COMAP_CW(KK) k_ds_compact_walk<NB, KK><<<(unsigned)((NO + 15) / 16), 256, 0, st>>>(                     \
        d->orow, s.cnt_nat, NO, L, npix, (const SlotRec<KK> *)s.srec, d->opix, d->ocnt, s.ekey, s.evn)
        if (s.KW == 1) { COMAP_NB_SWITCH(nb, COMAP_CW(1)); }
        else if (s.KW == 2) { COMAP_NB_SWITCH(nb, COMAP_CW(2)); }
        else { COMAP_NB_SWITCH(nb, COMAP_CW(4)); }
#undef COMAP_CW
    } else if (d->cf) {
        COMAP_NB_SWITCH(nb, (k_ds_compact_cf<NB><<<(unsigned)((NO + 3) / 4), 256, 0, st>>>(
                                d->orow, NO, L, npix, s.eval, s.eoff, d->opix, d->ocnt, s.ekey, s.epay)));
    } else {
        rows_fill(s.in, st, d->orow, d->opix, d->ow, s.ekey, s.eval, s.eoff);
    }
    COMAP_LAUNCH_CHECK(ctx);
    if (d->sell) {
        if (dalloc(ctx, &d->spix, d->nsell)) return -2;
        if (d->cf ? dalloc(ctx, (uint8_t **)&d->sco, d->nsell * nb) : dalloc(ctx, (double **)&d->sco, d->nsell * nb))
            return -2;
        const unsigned nch = (unsigned)((NO + 63) / 64);
        if (d->cf) {
            COMAP_NB_SWITCH(nb, (k_sell_fill_lds<NB, true><<<nch, 256, 0, st>>>(
                                    d->orow, d->opix, d->ocnt, d->sbase, NO, d->spix, d->sco)));
        } else {
            COMAP_NB_SWITCH(nb, (k_sell_fill_lds<NB, false><<<nch, 256, 0, st>>>(
                                    d->orow, d->opix, d->ow, d->sbase, NO, d->spix, d->sco)));
        }
        COMAP_LAUNCH_CHECK(ctx);
    }
    return 0;
}

// ---- 4. pixel-major transpose (stable: offset order within a pixel), the non-empty row list
static int phase4_transpose(comap_destriper *d, Setup &s, hipStream_t st)
{
    comap_ctx *ctx = d->ctx;
    const int64_t npix = d->npix;
    const int nb = d->nb;
    if (d->walk) {
        size_t tb = s.cub_tb;
        COMAP_CHECK(ctx, sort_pairs_i32(false, s.cub_tmp, tb, s.ekey, s.ekey2, s.evn, s.evn2, d->nnz, s.end_bit, st));
    } else if (d->cf) {
        COMAP_CHECK(ctx, hipcub::DeviceRadixSort::SortPairs(s.cub_tmp, s.sort64_tb, s.ekey, s.ekey2, s.epay, s.epay2,
                                                            (int)d->nnz, 0, s.end_bit, st));
    } else {
        COMAP_CHECK(ctx, hipcub::DeviceRadixSort::SortPairs(s.cub_tmp, s.sort_tb, s.ekey, s.ekey2, s.eval, s.eval2,
                                                            (int)d->nnz, 0, s.end_bit, st));
    }
    k_rowptr<<<grid_for(npix + 1), 256, 0, st>>>(s.ekey2, d->nnz, npix, d->prow);
    COMAP_LAUNCH_CHECK(ctx);
    if (d->walk) {   // (the sample walk of phase 5 writes the pixel-major offsets / counts)
    } else if (d->cf) {
        COMAP_NB_SWITCH(nb, k_pixel_entries_cf<NB><<<grid_for(d->nnz, 8192), 256, 0, st>>>(s.epay2, d->prow + npix,
                                                                                            d->poff, d->pcnt));
    } else {
        COMAP_NB_SWITCH(nb, k_pixel_entries<NB><<<grid_for(d->nnz, 8192), 256, 0, st>>>(s.eval2, d->prow + npix, s.eoff,
                                                                                         d->ow, d->poff, d->pw));
    }
    COMAP_LAUNCH_CHECK(ctx);
    k_hit_flags<<<grid_for(npix), 256, 0, st>>>(d->prow, npix, s.hflag, nb, s.hextra, d->walk ? d->h : nullptr, d->hits,
                                                d->nnum, s.counts);
    COMAP_LAUNCH_CHECK(ctx);
    COMAP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(s.cub_tmp, s.scan32_tb, s.hflag, s.hpos, (int)npix, st));
    // the walk's heavy rows: more entries than COMAP_DS_HEAVY (the Lissajous turn-round pixels hold
    // up to ~100x the mean; walked last they set the kernel's tail)
    k_hit_rows<<<grid_for(npix), 256, 0, st>>>(d->prow, s.hflag, s.hpos, npix, d->hrow, d->hprow, s.counts,
                                               d->opt.heavy, d->walk && d->opt.heavy > 0 ? s.hheavy : nullptr);
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

// ---- 5. sample-level maps (binValues order)
static int phase5_sample_maps(comap_destriper *d, Setup &s, hipStream_t st)
{
    comap_ctx *ctx = d->ctx;
    const int64_t N = d->N, NO = d->NO, npix = d->npix;
    const int L = d->L, nb = d->nb;
    const unsigned wgrid = (unsigned)std::min<int64_t>((npix + 3) / 4, 65536);
    if (d->walk) {
        if (s.kint) {
            k_keep_bits<<<grid_for(NO, 8192), 256, 0, st>>>(s.keep, d->perm, NO, nb, s.kint);
            COMAP_LAUNCH_CHECK(ctx);
        }
        // member slots per lane and chunk: 64 KW (one entry's members fit a chunk); one wave per
        // row (a fixed 2048-block grid: C5 0.80 -> 1.04 ms)
#define COMAP_W2(KK) k_sample_walk2<NB, KK, KK><<<wgrid, 256, 0, st>>>(                                              \
        d->hrow, d->hprow, s.counts, s.evn2, (const SlotRec<KK> *)s.srec, d->perm, d->wbar, s.in.w, s.payload, N, npix, \
        L, NO, s.kint, s.hextra, d->h, d->hits, d->nnum, d->poff, d->pcnt, d->opt.heavy > 0 ? s.hheavy : nullptr,   \
        d->opt.heavy)
        if (s.KW == 1) { COMAP_NB_SWITCH(nb, COMAP_W2(1)); }
        else if (s.KW == 2) { COMAP_NB_SWITCH(nb, COMAP_W2(2)); }
        else { COMAP_NB_SWITCH(nb, COMAP_W2(4)); }
#undef COMAP_W2
    } else {
        COMAP_CHECK(ctx, hipcub::DeviceRadixSort::SortPairs(s.cub_tmp, s.sort_tb, s.skey, s.skey2, s.sval, s.sval2, (int)N,
                                                            0, s.end_bit, st));
        k_rowptr<<<grid_for(npix + 1), 256, 0, st>>>(s.skey2, N, npix, s.srow);
        COMAP_LAUNCH_CHECK(ctx);
        COMAP_NB_SWITCH(nb, k_sample_walk<NB><<<wgrid, 256, 0, st>>>(s.srow, s.sval2, s.payload, npix, L, NO, s.keep, d->h,
                                                                     d->hits, d->nnum));
    }
    COMAP_LAUNCH_CHECK(ctx);
    return 0;
}

// Set-up of the constant operator (pointing and weights do not change during CG):
//   1. spatial offset order: first on-map pixel per offset, stable radix sort -> perm
//   2. k_ds_rows count pass: kept entries per row, ws / tw, the sample sort keys and
//      the packed sample payload; scan -> orow; nnz back to the host (sync 1)
//   3. k_ds_rows fill pass: the offset-major entries + the transpose's keys
//   4. pixel-major transpose: stable radix sort of the entries by pixel, row pointers,
//      gathered entry weights, the non-empty row list
//   5. sample-level maps: stable radix sort of the samples by pixel, ordered walk
//   nnzp and the non-empty row count back to the host (sync 2).
// The count form (cf), and with it the member-mask walk, replace the fill pass by a
// compaction of the count pass's slots and the sample sort by a walk of the transpose.
extern "C" int comap_destripe_create_bands(comap_ctx *ctx, const int32_t *pix, const double *tod, const double *w,
                                           const uint8_t *keep, int64_t N, int32_t L, int64_t npix, int32_t nb,
                                           comap_destriper **out)
{
    return comap_destripe_create_keyed(ctx, pix, tod, w, keep, nullptr, 0, N, L, npix, nb, out);
}

extern "C" int comap_destripe_create(comap_ctx *ctx, const int32_t *pix, const double *tod, const double *w,
                                     int64_t N, int32_t L, int64_t npix, comap_destriper **out)
{
    return comap_destripe_create_bands(ctx, pix, tod, w, nullptr, N, L, npix, 1, out);
}

extern "C" int comap_destripe_create_keyed(comap_ctx *ctx, const int32_t *pix, const double *tod, const double *w,
                                           const uint8_t *keep, const int32_t *okey, int64_t okey_max, int64_t N,
                                           int32_t L, int64_t npix, int32_t nb, comap_destriper **out)
{
    if (!ctx || !pix || !tod || !w || !out) return -1;
    COMAP_DEVICE_GUARD(ctx);
    *out = nullptr;
    if (nb != 1 && nb != 2 && nb != 4) return comap_fail(ctx, -1, "bands per problem must be 1, 2 or 4");
    if (L < 1 || L > 256) return comap_fail(ctx, -1, "offset_length must be in [1, 256]");
    if (N <= 0 || N % L) return comap_fail(ctx, -1, "n_samples must be a positive multiple of offset_length");
    // (npix below the SELL padding id's magnitude, so no pixel id in [-npix, npix) is the pad)
    if (npix <= 0 || npix >= 0x7f7f7f7fll || N >= (1ll << 31)) return comap_fail(ctx, -1, "size limits exceeded");
    hipStream_t st = ctx->stream;
    auto *d = new comap_destriper();
    d->ctx = ctx; d->N = N; d->L = L; d->NO = N / L; d->npix = npix; d->nb = nb;
    d->opt = read_options();
    d->walk = d->opt.walk;
    const int64_t NO = d->NO;
    const size_t NB = (size_t)nb;
    // destroys a partly built problem on every early return; released at the end
    std::unique_ptr<comap_destriper, int (*)(comap_destriper *)> own(d, comap_destripe_destroy);
    int rc = 0;
    rc |= dalloc(ctx, &d->orow, NO + 1);
    for (double **p : {&d->ws, &d->tw, &d->wbar, &d->pt}) rc |= dalloc(ctx, p, NO * NB);
    rc |= dalloc(ctx, &d->prow, npix + 1);
    for (double **p : {&d->h, &d->hits, &d->nnum}) rc |= dalloc(ctx, p, npix * NB);
    rc |= dalloc(ctx, &d->part, 2 * NB * (size_t)kPartMax);   // [0, NB kPartMax): p.q / dots, then r.r of the fused CG
    rc |= dalloc(ctx, &d->scal, 4 * NB + 4);
    rc |= dalloc(ctx, &d->hrow, npix);
    rc |= dalloc(ctx, &d->hprow, npix + 1);
    rc |= dalloc(ctx, &d->perm, NO);
    if (rc) return -2;
    if (okey && (okey_max < 1 || okey_max >= (1ll << 31))) return comap_fail(ctx, -1, "okey_max must be in [1, 2^31)");
    Setup s{{pix, w, tod, N, NO, npix, L, nb, d->perm}, keep, okey};
    while ((1ll << s.end_bit) <= npix) ++s.end_bit;
    while ((1ll << s.key_bit) <= (okey ? okey_max - 1 : npix)) ++s.key_bit;
    s.KW = L <= 64 ? 1 : (L <= 128 ? 2 : 4);
    // ---- scratch: one allocation, sized by a dry run of the layout
    Arena ar;
    ar.st = st;
    layout(ar, s, d, st);
    ar.cap = std::exchange(ar.used, 0);
    COMAP_CHECK(ctx, comap_tmp_alloc((void **)&ar.base, ar.cap, st));
    layout(ar, s, d, st);
    if (ar.used > ar.cap) return comap_fail(ctx, -2, "set-up scratch layout exceeds its allocation");
    COMAP_CHECK(ctx, comap_pinned_alloc((void **)&s.hw, 8 * 8));
    std::unique_ptr<int64_t, void (*)(void *)> hw_free(s.hw, comap_pinned_free);
    if ((rc = phase1_order(d, s, st))) return rc;
    if ((rc = phase2_count(d, s, st))) return rc;
    if ((rc = read_back_sizes(d, s, st))) return rc;
    if ((rc = phase3_fill(d, s, st))) return rc;
    if ((rc = phase4_transpose(d, s, st))) return rc;
    if ((rc = phase5_sample_maps(d, s, st))) return rc;
    // read-back 2 (sync 2): nnzp and the non-empty row count
    COMAP_CHECK(ctx, hipMemcpyAsync(s.hw, s.counts, 16, hipMemcpyDeviceToHost, st));
    COMAP_CHECK(ctx, hipStreamSynchronize(st));
    d->nnzp = s.hw[0];
    d->nh = s.hw[1];
    own.release();
    *out = d;
    return 0;
}
