// destriper_internal.h -- what the destriper's translation units share: the problem (struct
// comap_destriper), constants, launch helpers and device helpers of destriper_setup.hip (operator
// set-up), destriper_cg.hip (CG kernels, solve loop, accessors) and destriper_keys.hip (relabel keys),
// and the sorted-segments helper of destriper_segments.hip that destriper_ground.hip (ground set-up),
// destriper_split.hip (split maps) and destriper_resid.hip (residual group stage) sum by.
//
// Destriping map-maker (reference MapMaking/Destriper.py:85-263, 402-503).
//
// The reference's matvec A x = F^T W Z F x (op_Ax) bins every sample twice
// per call (binFuncs.binValues, 97% of its time) and its BiCG calls it three
// times per iteration with bit-identical arguments (p == pb, r == rb).
//
// Pointing and weights are constant during CG, so the operator is rebuilt
// here once as a sparse offset<->pixel structure:
//   entry (o, p, s) with s = sum of w_i over the samples i of offset o that
//   fall in pixel p.  Then, with ws_o = sum_{i in o} w_i and h = weight map,
//     num = W x               num_p = sum_{e in pixel row p} s_e x_{o(e)}
//     m   = num / h           (m_p = num_p where h_p == 0, as share_map)
//     y_o = ws_o x_o - sum_{e in offset row o} s_e m_{p(e)}      (op_Z + F^T W)
// Off-map samples (negative pixel ids p >= -npix) are never binned but gather m[npix + p],
// numpy's index wrap in the reference's m[pointing] (Destriper.py:211; -1 reads the last
// pixel); ids < -npix are rejected as numpy raises there.  One CG iteration streams
// 2 nnz entries instead of 6 N samples; all reductions are fixed-order
// (deterministic).  The sample-level maps (weight map h, hits, naive
// numerator sum w tod) are summed per pixel in sample order after a stable
// radix sort, i.e. in exactly binValues' order (bit-exact on one rank).
//
// Bands.  run_destriper.py:146-189 solves the 4 sidebands one after the other
// on the SAME pointing (only tod and weights differ per band).  A problem here
// holds NB in {1, 2, 4} bands as one batched system: the index structure
// (offset rows, pixel ids, pixel-major transpose) is shared and every per-band
// quantity is interleaved band-fastest -- entry weights [nnz][NB], CG vectors
// [N/L][NB], maps [npix][NB] -- so one entry-index load and one 8 NB-byte
// gather serve all bands, and one launch sequence advances every band's CG.
// Each band keeps its own scalars and stop flag (its iterates and iteration
// count are those of a separate solve).  An offset that a band's data prep
// drops (all weights zero, COMAPData.py:550-568) is marked in the per-band
// keep mask: its weights are zero, so it adds exactly nothing to that band's
// operator, and its samples are left out of that band's hit map.
//
// Layout of the device scalars (k-major, so one collective sums NB values):
//   scal[0:NB] rr0, [NB:2NB] rr, [2NB:3NB] p.q, [3NB:4NB] rr_new, [4NB] threshold
//   flags[0] all bands stopped, [1] iterations while any band ran,
//   [2+b] band b stopped, [2+NB+b] band b's iterations
// (NB = 1 is the single-band layout rr0, rr, pq, rr_new, threshold / stop, iterations.)
#pragma once
#include "comap_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

// The COMAP_DS_* options, read once per create (read_options in destriper_setup.hip).  -1 / 0: not
// set or not a valid value -- the default, which may depend on the problem's size, holds.
struct comap_ds_options {
    int sell = -1;          // COMAP_DS_SELL: 1 / 0 = sliced-ELLPACK projection on / off
    bool cf = true;         // COMAP_DS_CF=0: always the f64 entry weights
    bool walk = true;       // COMAP_DS_WALK=0: the sorted-sample payload walk
    int64_t heavy = 2048;   // COMAP_DS_HEAVY: entries above which the walk starts a row first (0: row order)
    int bin_lanes = 0;      // COMAP_DS_BL: lanes per pixel row (0: by the mean row length)
    int bin_u = 0;          // COMAP_DS_BU: entry loads in flight per bin lane
    int proj_lanes = 0;     // COMAP_DS_PG: lanes per offset row (0: by the mean row length)
    int proj_blocks = 0;    // COMAP_DS_PB: projection grid cap
    int cg_graph = -1;      // COMAP_DS_CGGRAPH: 1 / 0 = replay a captured graph or not (-1: by size)
};

struct comap_destriper {
    comap_ctx *ctx = nullptr;
    int64_t N = 0, NO = 0, npix = 0;
    int32_t L = 0;
    int32_t nb = 1;        // bands solved together (interleaved, band fastest)
    int64_t nnz = 0;       // offset-major entries (incl. off-map gathers)
    int64_t nnzp = 0;      // pixel-major entries (binned only)
    // offset-major
    int64_t *orow = nullptr;   // [NO+1]
    int32_t *opix = nullptr;   // [nnz]  pixel (-1 = off-map)
    double *ow = nullptr;      // [nnz][nb]
    double *ws = nullptr;      // [NO][nb] sum w
    double *tw = nullptr;      // [NO][nb] sum w tod
    // pixel-major
    int64_t *prow = nullptr;   // [npix+1]
    int32_t *poff = nullptr;   // [nnzp]
    double *pw = nullptr;      // [nnzp][nb]
    // count form (cf): every offset's non-zero sample weights in band b equal one value
    // wbar[o][b] (COMAP's weights are per (feed, band, file), cuts set 0), so an entry
    // stores the number of non-zero-weight samples per band (uint8) instead of the f64
    // sums: s_e = wbar_o c_e.  opix / poff + ocnt / pcnt replace ow / pw (4 + NB bytes per
    // entry instead of 4 + 8 NB); the bin gathers pt = wbar o x (written by the direction
    // kernel, or by k_scale), the projection multiplies its row sum by wbar_o.
    bool cf = false;
    comap_ds_options opt;      // the COMAP_DS_* options as they stood at create
    // launch shapes the set-up resolves from the options and the problem's size
    int bin_u = 4;             // entry loads in flight per bin lane
    int64_t proj_blocks = 1024;   // projection grid cap (its p.q partials are re-summed by every update block)
    // sliced-ELLPACK copy of the offset-major rows for the projection (COMAP_DS_SELL): chunk c
    // = 64 consecutive offsets (one wave, lane = offset), padded to its longest row and stored
    // column-major -- entry j of lane l at sbase[c] + 64 j + l -- so a lane streams its row
    // with coalesced loads, no row-pointer load and no cross-lane reduction
    bool sell = false;
    bool walk = false;         // sample-level maps by the member-mask walk (set-up; cleared when it fell back)
    int64_t nsell = 0;         // padded entries
    int64_t *sbase = nullptr;  // [NC + 1]
    int32_t *spix = nullptr;   // [nsell] pixel, -1 off-map, kSellPad padding
    void *sco = nullptr;       // [nsell][nb] counts (uint8) or weights (f64)
    uint8_t *ocnt = nullptr;   // [nnz][nb]
    uint8_t *pcnt = nullptr;   // [nnzp][nb]
    double *wbar = nullptr;    // [NO][nb]
    double *pt = nullptr;      // [NO][nb] scaled bin input (CG direction / scratch)
    // sample-level maps (local), [npix][nb]
    double *h = nullptr, *hits = nullptr, *nnum = nullptr;
    // reduction scratch
    double *part = nullptr;    // [2 nb kPartMax] block partials (band b at b kPartMax)
    double *scal = nullptr;    // [4 nb + 1] device scalars (layout above)
    // device-resident CG of comap_destripe_solve (fixed pointers: graph-replayable)
    double *cg = nullptr;          // [(4 NO + npix) nb]: x, r, p, q | num
    int32_t *flags = nullptr;      // [2 + 2 nb]
    int32_t *hrow = nullptr;       // [nh] pixel rows with entries (the CG bin skips empty rows)
    int64_t *hprow = nullptr;      // [nh + 1] their entry ranges: hprow[i] = prow[hrow[i]] (no empty row between)
    int64_t nh = 0;
    int32_t *perm = nullptr;       // [NO] internal offset position -> caller's offset
    int32_t *flags_host = nullptr; // pinned [2 + 2 nb]
    double *thr_host = nullptr;    // pinned [1 + 4 nb]: threshold, then a copy of scal's rr0 .. rr_new
    hipStream_t cs = nullptr;      // CG stream (graph capture needs a non-default stream)
    hipEvent_t ev = nullptr;
    hipGraphExec_t batch = nullptr;   // kCgBatch iterations
    // solve-mask view (destriper_mask.hip): a view borrows its parent's index structure, wbar and hits and
    // owns its coefficients, ws / tw, h / nnum, pt and CG state; a parent counts its live views
    comap_destriper *parent = nullptr;
    int nviews = 0;
};

constexpr int kProjU = 4;         // entry loads in flight per k_ds_project lane
constexpr int kProjBlocks = 1024; // k_ds_project grid cap: its p.q partials are re-summed by every update block
constexpr int kPartMax = 8192;     // >= every reduction grid of the CG unit
constexpr int kRedBlocks = 256;    // dot-product grids (k_dot_part)
constexpr int kCgBatch = 16;       // CG iterations per replayed graph (one host check per batch)
constexpr int64_t kSellMinOffsets = 131072;   // sliced-ELLPACK projection by default from this many offsets
constexpr int32_t kSellPad = (int32_t)0x80808080;   // memset pattern 0x80: a padding slot

typedef double d2v __attribute__((ext_vector_type(2)));

// v[0..NB) = p[0..NB) (16-B loads when NB is even; p is 8 NB-byte aligned)
template <int NB>
__device__ __forceinline__ void ldb(const double *__restrict__ p, double (&v)[NB])
{
    if constexpr (NB % 2 == 0) {
#pragma unroll
        for (int b = 0; b < NB; b += 2) {
            const d2v t = *reinterpret_cast<const d2v *>(p + b);
            v[b] = t.x;
            v[b + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int b = 0; b < NB; ++b) v[b] = p[b];
    }
}

template <int NB>
__device__ __forceinline__ void stb(double *__restrict__ p, const double (&v)[NB])
{
    if constexpr (NB % 2 == 0) {
#pragma unroll
        for (int b = 0; b < NB; b += 2) {
            d2v t;
            t.x = v[b];
            t.y = v[b + 1];
            *reinterpret_cast<d2v *>(p + b) = t;
        }
    } else {
#pragma unroll
        for (int b = 0; b < NB; ++b) p[b] = v[b];
    }
}

// One entry's coefficients held in registers between its load and its use (the bin's
// software pipeline): the count form keeps the packed uint8 counts (one dword for up to
// 4 bands), the full form the NB doubles.
template <int NB, bool CF>
struct Coef;
template <int NB>
struct Coef<NB, true> {
    uint32_t v = 0;
    __device__ __forceinline__ void load(const void *__restrict__ base, int64_t k)
    {
        const uint8_t *c = reinterpret_cast<const uint8_t *>(base) + k * NB;
        if constexpr (NB == 4) v = *reinterpret_cast<const uint32_t *>(c);
        else if constexpr (NB == 2) v = *reinterpret_cast<const uint16_t *>(c);
        else v = *c;
    }
    __device__ __forceinline__ double get(int b) const { return (double)((v >> (8 * b)) & 0xffu); }
};
template <int NB>
struct Coef<NB, false> {
    double v[NB] = {};
    __device__ __forceinline__ void load(const void *__restrict__ base, int64_t k)
    {
        ldb<NB>(reinterpret_cast<const double *>(base) + k * NB, v);
    }
    __device__ __forceinline__ double get(int b) const { return v[b]; }
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Fixed-order sum of n block partials by one 256-thread block (k_dot_final's order).
// Each thread adds part[tid], part[tid + 256], ... in that order; the loads are issued
// 8 at a time before the adds (a serial load -> add chain costs one L2 round trip per
// partial: ~40 us for 4 bands x 2k partials at C4, most of the CG update kernel).
__device__ __forceinline__ double block_final_sum(const double *__restrict__ part, int n, double *red)
{
    double acc = 0.0;
    constexpr int kB = 8;
    int i = threadIdx.x;
    for (; i + (kB - 1) * 256 < n; i += kB * 256) {
        double v[kB];
#pragma unroll
        for (int k = 0; k < kB; ++k) v[k] = part[i + k * 256];
#pragma unroll
        for (int k = 0; k < kB; ++k) acc += v[k];
    }
    for (; i < n; i += 256) acc += part[i];
    acc = wave_sum(acc);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// one offset's x += a p ; r -= a q for the live bands, accumulating r.r (16-B vector access)
template <int NB>
__device__ __forceinline__ void update_row(double *__restrict__ x, double *__restrict__ r, const double *__restrict__ p,
                                           const double *__restrict__ q, const double (&a)[NB], const bool (&live)[NB],
                                           double (&acc)[NB])
{
    double xv[NB], rv[NB], pv[NB], qv[NB];
    ldb<NB>(r, rv);
    ldb<NB>(p, pv);
    ldb<NB>(q, qv);
    ldb<NB>(x, xv);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (live[b]) {
            xv[b] += a[b] * pv[b];
            rv[b] = rv[b] - a[b] * qv[b];
        }
        acc[b] = fma(rv[b], rv[b], acc[b]);
    }
    stb<NB>(x, xv);
    stb<NB>(r, rv);
}

// p = r + beta p for the live bands of one offset; wbar != NULL (count form): also
// pt = wbar o p, the next bin's input
template <int NB>
__device__ __forceinline__ void direction_row(double *__restrict__ p, const double *__restrict__ r,
                                              const double (&beta)[NB], const bool (&live)[NB],
                                              const double *__restrict__ wbar = nullptr, double *__restrict__ pt = nullptr)
{
    double pv[NB], rv[NB];
    ldb<NB>(p, pv);
    ldb<NB>(r, rv);
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if (live[b]) pv[b] = rv[b] + beta[b] * pv[b];
    stb<NB>(p, pv);
    if (wbar) {
        double a[NB];
        ldb<NB>(wbar, a);
#pragma unroll
        for (int b = 0; b < NB; ++b) pv[b] *= a[b];
        stb<NB>(pt, pv);
    }
}

// Wave sums of V values per lane (V a power of two <= 64) by a reduce-scatter butterfly:
// the first log2 V steps exchange half of the remaining values (each lane keeps the half
// its lane bit selects), the rest reduce the single value left, so V sums cost V - 1 + 6 -
// log2 V exchanges instead of 6 V.  Afterwards x[0] holds value lane / (64 / V)'s total (a
// fixed order; a + b == b + a, so both lanes of a pair hold the same bits).
template <int V>
__device__ __forceinline__ void wave_sum_scatter(double (&x)[V], int lane)
{
    // (values held in named registers and selected as values: a select between two array
    // elements was turned into a lane-dependent index, i.e. v_cndmask chains over all V)
    static_assert(V == 2 || V == 4 || V == 8, "V");
    double y[V];
#pragma unroll
    for (int j = 0; j < V; ++j) y[j] = x[j];
    int sft = 32;
    if constexpr (V >= 8) {
        const bool up = (lane & sft) != 0;
        const double s0 = up ? y[0] : y[4], s1 = up ? y[1] : y[5], s2 = up ? y[2] : y[6], s3 = up ? y[3] : y[7];
        const double k0 = up ? y[4] : y[0], k1 = up ? y[5] : y[1], k2 = up ? y[6] : y[2], k3 = up ? y[7] : y[3];
        y[0] = k0 + __shfl_xor(s0, sft, 64);
        y[1] = k1 + __shfl_xor(s1, sft, 64);
        y[2] = k2 + __shfl_xor(s2, sft, 64);
        y[3] = k3 + __shfl_xor(s3, sft, 64);
        sft >>= 1;
    }
    if constexpr (V >= 4) {
        const bool up = (lane & sft) != 0;
        const double s0 = up ? y[0] : y[2], s1 = up ? y[1] : y[3];
        const double k0 = up ? y[2] : y[0], k1 = up ? y[3] : y[1];
        y[0] = k0 + __shfl_xor(s0, sft, 64);
        y[1] = k1 + __shfl_xor(s1, sft, 64);
        sft >>= 1;
    }
    {
        const bool up = (lane & sft) != 0;
        const double s0 = up ? y[0] : y[1], k0 = up ? y[1] : y[0];
        y[0] = k0 + __shfl_xor(s0, sft, 64);
        sft >>= 1;
    }
#pragma unroll
    for (int o = 32 / V; o > 0; o >>= 1) y[0] += __shfl_xor(y[0], o, 64);
    x[0] = y[0];
}

// v of lane `src` (wave-uniform) by two v_readlane
__device__ __forceinline__ double read_lane(double v, int src)
{
    const uint64_t u = __double_as_longlong(v);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, src), hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), src);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

inline unsigned grid_for(int64_t n, int64_t cap = 4096) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap)); }

// every templated launch dispatches on the problem's band count (1, 2 or 4)
#define COMAP_NB_SWITCH(nb, ...)                                 \
    switch (nb) {                                                \
    case 1: { constexpr int NB = 1; __VA_ARGS__; } break;       \
    case 2: { constexpr int NB = 2; __VA_ARGS__; } break;       \
    default: { constexpr int NB = 4; __VA_ARGS__; } break;      \
    }

// destriper_cg.hip's launchers as the ground solve (destriper_ground.hip) uses them: one band, on
// the problem's CG stream, scalars (d->scal), stop flags (d->flags) and partials (d->part).
//   ds_cg_state        the CG stream, event, stop flags and pinned read-back blocks (no vectors)
//   ds_cg_use_graph    COMAP_DS_CGGRAPH / the size rule of the plain solve
//   ds_launch_bin / ds_launch_project   the plain problem's bin and projection
//   ds_dot             out = a . b over n values
//   ds_dot_part        k_dot_part alone: kRedBlocks block partials of a . b in d->part
//   ds_upd_grid        the CG update's grid (hence its r.r partials) for NO offsets
//   ds_div_map         out_p = num_p / h_p (num_p where h_p == 0) over n values
int ds_cg_state(comap_destriper *d);
bool ds_cg_use_graph(const comap_destriper *d);
void ds_launch_bin(const comap_destriper *d, hipStream_t st, const double *x, const double *base, const double *hdiv,
                   double *num, const int32_t *flags, bool hit_rows, bool x_scaled);
void ds_launch_project(const comap_destriper *d, hipStream_t st, const double *x, const double *num, const double *h,
                       double *y, const int32_t *flags);
void ds_dot(comap_destriper *d, hipStream_t st, const double *a, const double *b, int64_t n, double *out);
void ds_dot_part(comap_destriper *d, hipStream_t st, const double *a, const double *b, int64_t n);
unsigned ds_upd_grid(int64_t NO);
void ds_div_map(hipStream_t st, const double *num, const double *h, int64_t n, double *out);
// ... and the native solve's own four launches as the prior solve (destriper_prior.hip) enqueues them,
// one band, on the problem's scalars, stop flags and partials (p.q at d->part, r.r at d->part + kPartMax):
//   ds_launch_project_parts    the projection from the divided map, its p.q block partials in d->part;
//                              returns its grid (= the partials written)
//   ds_launch_update_fused     k_cg_update_fused over the first npq partials of d->part
//   ds_launch_direction_fused  k_cg_direction_fused (count form: it also writes d->pt)
//   ds_scale                   xs = wbar o x (the count form's bin input)
//   ds_unpermute               out[perm[k]] = x[k]
unsigned ds_launch_project_parts(const comap_destriper *d, hipStream_t st, const double *x, const double *num,
                                 double *y, const int32_t *flags);
void ds_launch_update_fused(const comap_destriper *d, hipStream_t st, int npq, double *x, double *r, const double *p,
                            const double *q, const int32_t *flags);
void ds_launch_direction_fused(const comap_destriper *d, hipStream_t st, double *p, const double *r, int32_t *flags);
void ds_scale(const comap_destriper *d, hipStream_t st, const double *x, double *xs);
void ds_unpermute(const comap_destriper *d, hipStream_t st, const double *x, double *out);

inline int bits_for(uint64_t bound)   // bits that hold every key in [0, bound)
{
    int b = 1;
    while (b < 64 && (uint64_t(1) << b) < bound) ++b;
    return b;
}

// Sorted segments (destriper_segments.hip): the n caller-made keys (Key = uint32_t or uint64_t)
// sorted stably over `bits` bits with their indices, cut into ne segments of equal key -- segment e
// is the sorted positions [estart[e], estart[e + 1]), n behind the last -- and the caller's two
// device flag words, read back with the segment count in the call's one host wait.  The buffers
// come from the caller's DevTemps and live as long as it does.
template <typename Key>
struct ds_segments {
    Key *skey = nullptr;                          // [n] sorted keys
    int32_t *sval = nullptr, *estart = nullptr;   // [n] sorted indices, [ne] segment starts
    int64_t ne = 0;
    int64_t flag[2] = {0, 0};
};
template <typename Key>
int ds_sorted_segments(comap_ctx *ctx, DevTemps &tmp, const Key *key, int64_t n, int bits, const int32_t *flag,
                       ds_segments<Key> *out);

// a problem's persistent buffers come from the cached device pool (comap_tmp_alloc) in
// the context stream's order; comap_destripe_destroy returns them after a device sync
template <typename T>
int dalloc(comap_ctx *ctx, T **p, size_t n)
{
    void *q = nullptr;
    COMAP_CHECK(ctx, comap_tmp_alloc(&q, sizeof(T) * (n ? n : 1), ctx->stream));
    *p = (T *)q;
    return 0;
}
