// intersect.hip — Deps.intersecting(scope) of merged deps for every (destination, request) pair
// (ad_deps_intersect; Deps.java:205-218): the coordinator's Accept / Commit / Apply carry
// deps.intersecting(route.slice(rangesForNode(to))), three times per transaction and replica.
//
// One group per (destination d, request r, map m). scope(r, d) = route(r).slice(R_d) is never built: a key is in
// it when it is in the route and in a range of R_d, a range intersects it when it intersects route(r) inside a
// range of R_d -- two binary searches per tested key.
//   KEY / DIRECT_KEY  KeyDeps.intersecting / slice -> select (KeyDeps.java:189-248): the map's keys in the scope
//   RANGE             RangeDeps.intersecting(keys) (:611-621) / slice(ranges) (:594-609): the map's ranges that hold
//                     a scope key / intersect a scope range (Range.compareIntersecting, Range.java:296-305), whole
//                     (RangeCollector.copy, :833-842), in input order, each once
//   all               RelationMultiMap.trimUnusedValues (:491-532): txnIds trimmed to the ids still referenced,
//                     keysToTxnIds remapped
// A size pass and an emit pass around the offset scan (kernels.hip run_scan_arrays). A group is worked by one
// block: a wave (64 threads) for the common small maps, 256 threads for maps of more than IS_LIGHT_IDS ids or
// IS_LIGHT_K2T keysToTxnIds ints (listed by the size pass). The ids a group keeps are a bitmap in LDS; an id's
// new index is the popcount below its bit.
#include "intersect.hpp"

#include <algorithm>

#include "wave.hpp"

namespace adx {

namespace {

constexpr uint32_t IS_LIGHT_IDS = 2048, IS_LIGHT_K2T = 4096;

template <int NT, int BW>
struct ILds {
    uint32_t bits[BW];         // ids referenced by a selected key
    uint32_t pre[BW];          // set bits before each word
    uint32_t dst[NT + 1];      // chunk of NT keys: exclusive prefix of the selected keys' list lengths
    uint32_t src[NT];          //                   start of each key's list in the input keysToTxnIds
    uint32_t wtot[NT / 64];
};

// the first i in [0, n) with p(i), p monotone (false.. true..); n when none
template <class P>
__device__ __forceinline__ uint32_t first_true(uint32_t n, P p)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi)
    {
        const uint32_t mid = (lo + hi) >> 1;
        if (p(mid)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// sorted, disjoint ranges {start[i * stride], end[i * stride]}
struct RangeList {
    const int64_t* start; const int64_t* end;
    uint32_t n, stride;
    __device__ __forceinline__ int64_t s(uint32_t i) const { return start[(uint64_t)i * stride]; }
    __device__ __forceinline__ int64_t e(uint32_t i) const { return end[(uint64_t)i * stride]; }
    // Range.contains(key) of some range, in the store's inclusivity
    __device__ __forceinline__ bool contains(int64_t k, bool si) const
    {
        const uint32_t i = first_true(n, [&](uint32_t j) { return si ? e(j) > k : e(j) >= k; });
        return i < n && (si ? s(i) <= k : s(i) < k);
    }
    // some range intersects the open interval (lo, hi) of bounds (compareIntersecting: inclusivity plays no part)
    __device__ __forceinline__ bool intersects(int64_t lo, int64_t hi) const
    {
        const uint32_t i = first_true(n, [&](uint32_t j) { return e(j) > lo; });
        return i < n && s(i) < hi;
    }
};

struct Group {
    uint32_t m, nk, ni, no;
    const int64_t* K;          // keys (ranges: 2 words)
    const int32_t* T;          // keysToTxnIds
    RangeList dest, rroute;
    const int64_t* rkeys; uint32_t n_rkeys;
    bool range_route, si;

    // is key / range i of the map selected by scope(r, d)?
    __device__ bool select(uint32_t i) const
    {
        if (m != 1)
        {
            const int64_t k = K[i];
            if (!dest.contains(k, si)) return false;
            if (range_route) return rroute.contains(k, si);
            const uint32_t j = first_true(n_rkeys, [&](uint32_t x) { return rkeys[x] >= k; });
            return j < n_rkeys && rkeys[j] == k;
        }
        const int64_t s = K[2 * (uint64_t)i], e = K[2 * (uint64_t)i + 1];
        // the ranges of R_d that intersect it; inside each, a route key it holds or a route range it intersects
        for (uint32_t b = first_true(dest.n, [&](uint32_t j) { return dest.e(j) > s; }); b < dest.n && dest.s(b) < e; ++b)
        {
            const int64_t bs = dest.s(b), be = dest.e(b), lo = s > bs ? s : bs, hi = e < be ? e : be;
            if (range_route)
            {
                if (rroute.intersects(lo, hi)) return true;
                continue;
            }
            const uint32_t j = first_true(n_rkeys, [&](uint32_t x) { return si ? rkeys[x] >= lo : rkeys[x] > lo; });
            if (j < n_rkeys && (si ? rkeys[j] < hi : rkeys[j] <= hi)) return true;
        }
        return false;
    }
};

template <int NT>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wtot, uint32_t* total)
{
    const uint32_t inc = wave_incl_scan_dpp(v);
    if constexpr (NT == 64)
    {
        *total = (uint32_t)__shfl((int)inc, 63, 64);
        return inc - v;
    }
    else
    {
        const uint32_t w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 63) wtot[w] = inc;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (uint32_t x = 0; x < NT / 64; ++x)
        {
            const uint32_t t = wtot[x];
            if (x < w) pre += t;
            tot += t;
        }
        __syncthreads();
        *total = tot;
        return pre + inc - v;
    }
}

// One pass over the map's keys in chunks of NT. Marking (WRITE false): the ids of the selected keys' lists into
// L.bits; returns the selected keys and the ints of their lists. Writing: the selected keys, their end offsets
// and their lists with every id index replaced by its rank among the marked ids (L.pre / L.bits).
template <int NT, int BW, bool WRITE>
__device__ void sweep(const Group& g, ILds<NT, BW>& L, uint32_t* error, uint32_t n_sel_out, int64_t* o_keys, int32_t* o_k2t,
                      uint32_t* n_sel, uint32_t* sel_len)
{
    const uint32_t tid = threadIdx.x;
    uint32_t sel_base = 0, len_base = 0;
    for (uint32_t base = 0; base < g.nk; base += NT)
    {
        const uint32_t i = base + tid;
        const bool s = i < g.nk && g.select(i);
        uint32_t start = 0, len = 0;
        if (s)
        {
            start = i == 0 ? g.nk : (uint32_t)g.T[i - 1];
            const uint32_t end = (uint32_t)g.T[i];
            if (start < g.nk || end < start || end > g.no) atomicOr(error, IS_E_INPUT);
            else len = end - start;
        }
        uint32_t tot, cnt;
        const uint32_t ex_len = block_excl_scan<NT>(len, L.wtot, &tot);
        const uint32_t ex_sel = block_excl_scan<NT>(s ? 1u : 0u, L.wtot, &cnt);
        L.dst[tid] = ex_len;
        L.src[tid] = start;
        if (tid == 0) L.dst[NT] = tot;
        if (WRITE && s)
        {
            const uint32_t j = sel_base + ex_sel;
            if (g.m == 1)
            {
                o_keys[2 * (uint64_t)j] = g.K[2 * (uint64_t)i];
                o_keys[2 * (uint64_t)j + 1] = g.K[2 * (uint64_t)i + 1];
            }
            else o_keys[j] = g.K[i];
            o_k2t[j] = (int32_t)(n_sel_out + len_base + ex_len + len);
        }
        __syncthreads();
        // the chunk's list ints, one per thread and step: its key is the last one whose prefix does not pass it
        for (uint32_t e = tid; e < tot; e += NT)
        {
            const uint32_t c = first_true((uint32_t)NT, [&](uint32_t x) { return L.dst[x + 1] > e; });
            const uint32_t v = (uint32_t)g.T[L.src[c] + (e - L.dst[c])];
            if (v >= g.ni)
            {
                atomicOr(error, IS_E_INPUT);
                continue;
            }
            if (WRITE) o_k2t[n_sel_out + len_base + e] = (int32_t)(L.pre[v >> 5] + __popc(L.bits[v >> 5] & ((1u << (v & 31)) - 1u)));
            else atomicOr(&L.bits[v >> 5], 1u << (v & 31));
        }
        __syncthreads();
        sel_base += cnt;
        len_base += tot;
    }
    *n_sel = sel_base;
    *sel_len = len_base;
}

// the ids marked in L.bits[0, W): L.pre, and their number
template <int NT, int BW>
__device__ uint32_t rank_ids(ILds<NT, BW>& L, uint32_t W)
{
    const uint32_t per = (W + NT - 1) / NT, b = threadIdx.x * per, e = min(b + per, W);
    uint32_t s = 0;
    for (uint32_t j = b; j < e; ++j) s += __popc(L.bits[j]);
    uint32_t used;
    uint32_t run = block_excl_scan<NT>(s, L.wtot, &used);
    for (uint32_t j = b; j < e; ++j)
    {
        L.pre[j] = run;
        run += __popc(L.bits[j]);
    }
    __syncthreads();
    return used;
}

__device__ __forceinline__ bool is_heavy(uint32_t ni, uint32_t no) { return ni > IS_LIGHT_IDS || no > IS_LIGHT_K2T; }

// the group g = 3 * row + m: its input map and scope; false when the block has nothing to do
template <bool HEAVY>
__device__ bool bind_group(const IntersectArgs& a, uint64_t gi, Group* g, uint64_t* row)
{
    const uint64_t rw = gi / 3, r = rw % a.n_owned;
    const uint32_t m = (uint32_t)(gi % 3), d = (uint32_t)(rw / a.n_owned);
    *row = rw;
    const uint64_t ko = a.keys_off[m][r], to = a.txn_off[m][r], oo = a.k2t_off[m][r];
    g->m = m;
    g->nk = (uint32_t)(a.keys_off[m][r + 1] - ko);
    g->ni = (uint32_t)(a.txn_off[m][r + 1] - to);
    g->no = (uint32_t)(a.k2t_off[m][r + 1] - oo);
    if (g->nk == 0 || is_heavy(g->ni, g->no) != HEAVY) return false;
    g->K = a.keys[m] + (m == 1 ? 2 : 1) * ko;
    g->T = a.k2t[m] + oo;
    const uint64_t d0 = a.dest_off[d];
    g->dest = RangeList{a.dest_start + d0, a.dest_end + d0, (uint32_t)(a.dest_off[d + 1] - d0), 1};
    const uint64_t r0 = a.route_off[r], r1 = a.route_off[r + 1];
    g->range_route = a.domain && a.domain[r];
    g->si = a.start_inclusive;
    const uint32_t words = r1 >= r0 ? (uint32_t)(r1 - r0) : 0;
    g->rkeys = a.route + r0;
    g->n_rkeys = words;
    g->rroute = RangeList{a.route + r0, a.route + r0 + 1, words / 2, 2};
    return true;
}

template <int NT, int BW, bool HEAVY>
__device__ void size_group(const IntersectArgs& a, uint64_t gi, ILds<NT, BW>& L)
{
    Group g;
    uint64_t row;
    const uint64_t N = (uint64_t)a.n_dest * a.n_owned;
    if (!bind_group<HEAVY>(a, gi, &g, &row))
    {
        if (!HEAVY && g.nk && threadIdx.x == 0) a.heavy[atomicAdd(a.n_heavy, 1u)] = (uint32_t)gi;
        return;
    }
    uint32_t out[3] = {0, 0, 0};
    if (g.ni > 32u * BW)
    {
        if (threadIdx.x == 0) atomicOr(a.error, IS_E_IDS);
    }
    else
    {
        const uint32_t W = (g.ni + 31) / 32;
        for (uint32_t j = threadIdx.x; j < W; j += NT) L.bits[j] = 0;
        __syncthreads();
        uint32_t n_sel, sel_len;
        sweep<NT, BW, false>(g, L, a.error, 0, nullptr, nullptr, &n_sel, &sel_len);
        const uint32_t used = rank_ids<NT, BW>(L, W);
        if (n_sel == g.nk)      // select.size() == keys.size(): `this` (KeyDeps.java:212, RangeDeps.java:628)
        {
            out[0] = g.nk; out[1] = g.ni; out[2] = g.no;
        }
        else if (n_sel)
        {
            out[0] = n_sel; out[1] = used; out[2] = n_sel + sel_len;
        }
    }
    if (threadIdx.x < 3) a.gsz[(3ull * threadIdx.x + g.m) * N + row] = out[threadIdx.x];
    __syncthreads();            // L is reused by the block's next group
}

template <class T>
__device__ __forceinline__ void copy_n(T* dst, const T* src, uint64_t n, uint32_t nt)
{
    for (uint64_t i = threadIdx.x; i < n; i += nt) dst[i] = src[i];
}

template <int NT, int BW, bool HEAVY>
__device__ void emit_group(const IntersectArgs& a, uint64_t gi, ILds<NT, BW>& L)
{
    Group g;
    uint64_t row;
    const uint64_t N = (uint64_t)a.n_dest * a.n_owned;
    if (!bind_group<HEAVY>(a, gi, &g, &row)) return;
    const uint64_t* ok = a.goff + (uint64_t)(0 + g.m) * (N + 1) + row;
    const uint64_t* oi = a.goff + (uint64_t)(3 + g.m) * (N + 1) + row;
    const uint64_t* ot = a.goff + (uint64_t)(6 + g.m) * (N + 1) + row;
    const uint32_t n_sel = (uint32_t)(ok[1] - ok[0]);
    if (n_sel == 0 || g.ni > 32u * BW) return;
    const uint64_t r = row % a.n_owned, to = a.txn_off[g.m][r];
    const uint32_t kw = g.m == 1 ? 2 : 1;
    int64_t* o_keys = a.o_keys[g.m] + kw * ok[0];
    int32_t* o_k2t = a.o_k2t[g.m] + ot[0];
    if (n_sel == g.nk)
    {
        copy_n(o_keys, g.K, (uint64_t)kw * g.nk, NT);
        copy_n(o_k2t, g.T, g.no, NT);
        if (a.rank_ids) copy_n((uint32_t*)a.o_ids[g.m] + oi[0], (const uint32_t*)a.txns[g.m] + to, g.ni, NT);
        else copy_n((int64_t*)a.o_ids[g.m] + 3 * oi[0], a.txns[g.m] + 3 * to, 3ull * g.ni, NT);
        return;
    }
    const uint32_t W = (g.ni + 31) / 32;
    for (uint32_t j = threadIdx.x; j < W; j += NT) L.bits[j] = 0;
    __syncthreads();
    uint32_t n1, l1;
    sweep<NT, BW, false>(g, L, a.error, 0, nullptr, nullptr, &n1, &l1);
    rank_ids<NT, BW>(L, W);
    sweep<NT, BW, true>(g, L, a.error, n_sel, o_keys, o_k2t, &n1, &l1);
    // trimUnusedValues: the marked ids, in order
    for (uint32_t v = threadIdx.x; v < g.ni; v += NT)
    {
        const uint32_t w = L.bits[v >> 5], bit = 1u << (v & 31);
        if (!(w & bit)) continue;
        const uint64_t j = oi[0] + L.pre[v >> 5] + __popc(w & (bit - 1u));
        if (a.rank_ids) ((uint32_t*)a.o_ids[g.m])[j] = ((const uint32_t*)a.txns[g.m])[to + v];
        else
        {
            const int64_t* s = a.txns[g.m] + 3 * (to + v);
            int64_t* o = (int64_t*)a.o_ids[g.m] + 3 * j;
            o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
        }
    }
    __syncthreads();            // L is reused by the block's next group
}

constexpr int NT_L = 64, BW_L = IS_LIGHT_IDS / 32, NT_H = 256, BW_H = IS_MAX_IDS / 32;

// the route CSR starts at 0 and ascends at r (else no group of the request is worked)
__device__ bool route_ok(const IntersectArgs& a, uint64_t gi)
{
    const uint64_t r = (gi / 3) % a.n_owned;
    const bool ok = a.route_off[0] == 0 && a.route_off[r] <= a.route_off[r + 1];
    if (!ok && threadIdx.x == 0) atomicOr(a.error, IS_E_ROUTE);
    return ok;
}

__global__ void __launch_bounds__(NT_L) k_isect_size(IntersectArgs a)
{
    __shared__ ILds<NT_L, BW_L> L;
    const uint64_t N = (uint64_t)a.n_dest * a.n_owned, gi = blockIdx.x;
    if (threadIdx.x < 3) a.gsz[(3ull * threadIdx.x + gi % 3) * N + gi / 3] = 0;
    if (!route_ok(a, gi)) return;
    size_group<NT_L, BW_L, false>(a, gi, L);
}

__global__ void __launch_bounds__(NT_H) k_isect_size_heavy(IntersectArgs a)
{
    __shared__ ILds<NT_H, BW_H> L;
    const uint32_t n = *a.n_heavy;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) size_group<NT_H, BW_H, true>(a, a.heavy[i], L);
}

__global__ void __launch_bounds__(NT_L) k_isect_emit(IntersectArgs a)
{
    __shared__ ILds<NT_L, BW_L> L;
    emit_group<NT_L, BW_L, false>(a, blockIdx.x, L);
}

__global__ void __launch_bounds__(NT_H) k_isect_emit_heavy(IntersectArgs a)
{
    __shared__ ILds<NT_H, BW_H> L;
    const uint32_t n = *a.n_heavy;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) emit_group<NT_H, BW_H, true>(a, a.heavy[i], L);
}

__global__ void k_isect_totals(IntersectArgs a, uint64_t* tot)
{
    const uint64_t N = (uint64_t)a.n_dest * a.n_owned;
    if (threadIdx.x < 9) tot[threadIdx.x] = a.goff[(uint64_t)threadIdx.x * (N + 1) + N];
    if (threadIdx.x == 9) tot[9] = *a.error;
    if (threadIdx.x == 10) tot[10] = *a.n_heavy;
}

constexpr unsigned HEAVY_GRID = 1024;

}  // namespace

hipError_t run_intersect_size(const IntersectArgs& a, hipStream_t st)
{
    const uint64_t G = 3ull * a.n_dest * a.n_owned;
    if (G == 0) return hipSuccess;
    k_isect_size<<<(unsigned)G, NT_L, 0, st>>>(a);
    k_isect_size_heavy<<<HEAVY_GRID, NT_H, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t run_intersect_totals(const IntersectArgs& a, uint64_t* tot, hipStream_t st)
{
    k_isect_totals<<<1, 64, 0, st>>>(a, tot);
    return hipGetLastError();
}

hipError_t run_intersect_emit(const IntersectArgs& a, uint32_t n_heavy, hipStream_t st)
{
    const uint64_t G = 3ull * a.n_dest * a.n_owned;
    if (G == 0) return hipSuccess;
    k_isect_emit<<<(unsigned)G, NT_L, 0, st>>>(a);
    if (n_heavy) k_isect_emit_heavy<<<std::min<unsigned>(n_heavy, HEAVY_GRID), NT_H, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace adx
