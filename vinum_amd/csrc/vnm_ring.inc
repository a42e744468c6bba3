// The LDS RING protocol of the ring-scatter kernels, once (included by vnm_agg.hip and vnm_sort.hip inside namespace vnm, before their
// first user).  fxn_scatter_kernel, pring_scatter_kernel, ssort_scatter_kernel and xsort_scatter_kernel are built on it;
// dring_scatter_kernel takes the level-2 region walk from here and keeps a copy of the rest (see there for why).
//
// Every partition has a ring of `cap` entries in LDS.  A sub-tile's entries are inserted with one LDS atomic each, whole blocks of FB
// entries leave for the partition's region in HBM (contiguous, aligned stores), and entries that found their ring full stay pending in
// their thread's registers for another insert / flush round of the same sub-tile.  The core owns the bookkeeping (RingState), the slot
// reservation, the walk over the rings and the round loop.  A kernel supplies its entry type and ring arrays, the partition of an
// entry, how a block is moved, and what happens when a region is full or the rounds run out -- as template constants, run-time values it
// has anyway, or callables.  Nothing here knows which kernel calls it.

// The bookkeeping of a kernel's rings: a view of six LDS arrays that the kernel declares ([np] unless noted).  They stay separate
// variables, not members of one LDS struct: the compiler keeps accesses to distinct LDS variables apart, the members of one variable it
// does not (fill[p] against head[q]) -- as one struct, ssort_scatter_kernel<true, 2> took two more registers and lost an occupancy step.
// HEAD: the type of a ring's head index -- 16 bits for ssort_scatter_kernel, which sits 1 KB below the 160 KB of LDS.
template <typename HEAD>
struct RingState {
    uint32_t* fill;       // entries in the ring (may run past cap: the inserts that found it full)
    HEAD* head;           // first occupied slot
    uint32_t* cursor;     // entries written to the partition's region so far
    uint32_t* retry;      // [2] a lane holds a pending entry after round k: retry[k & 1]
    uint32_t* nready;     // [2] the rings that completed a block in round k: nready[k & 1] of them, in ready[]
    // Every ring starts a round with less than one block (the flush takes all whole blocks), so it completes its first block of the
    // round exactly once: the lane whose entry is that block's last lists the ring, and the flush walks the list (~256 of 512 rings per
    // round of 4096 entries) instead of asking every ring for its fill (the sort's scatters: 4.5 -> 3.9 ms).  ONE list: a round's
    // inserts start after the barrier that ends the previous round's flush; only the counters alternate.
    uint16_t* ready;
};

// (all threads; MAXP: the length of the arrays; the caller's next barrier publishes it)
template <int BLOCK, int MAXP, typename HEAD>
__device__ __forceinline__ void ring_init(const RingState<HEAD>& st) {
    for (int i = threadIdx.x; i < MAXP; i += BLOCK) { st.fill[i] = 0; st.head[i] = 0; st.cursor[i] = 0; }
    if (threadIdx.x < 2) { st.retry[threadIdx.x] = 0; st.nready[threadIdx.x] = 0; }
}

// A slot for one entry in ring p, or RING_FULL (-1): the ring is full and the entry stays pending.  The caller stores its entry at
// [p * cap + slot].
constexpr uint32_t RING_FULL = ~0u;
template <int FB, typename HEAD>
__device__ __forceinline__ uint32_t ring_reserve(const RingState<HEAD>& st, int ph, uint32_t p, uint32_t cap, bool use_list) {
    const uint32_t r = atomicAdd(&st.fill[p], 1u);
    if (r == (uint32_t)FB - 1u && use_list) st.ready[atomicAdd(&st.nready[ph], 1u)] = (uint16_t)p;
    if (r >= cap) return RING_FULL;
    uint32_t slot = st.head[p] + r;
    if (slot >= cap) slot -= cap;
    return slot;
}

// Whole blocks of the listed rings (no list, or `drain`: of every ring; `drain`: the last, partial block as well -- end of the kernel)
// -> the partition's region, LANES lanes per ring.  For every block, every lane of the ring calls
//     move(p, src, dst, n_here, j, room)
// p: the partition; src: the block's first slot in the ring (wrapped); dst: its first entry index within the region (64 bits, cursor +
// offset: added to the caller's region base, base + cursor leaves the block loop -- as a 32-bit sum it cost ssort_scatter_kernel<false, 2>
// two registers and an occupancy step); n_here: its entries (< FB only when draining); j: the lane's number among the ring's LANES;
// room: the region takes a whole block at dst.  With room the caller moves the block; without, it applies its own policy (fail the
// attempt, spill).  Lane 0 rewrites the ring.
// RUN_ON: a block without room advances the region's cursor all the same (the sorts: the count shows the overflow, capped at ocap);
// otherwise the cursor counts what was written (the aggregates: the regions stay readable, the block went elsewhere).
template <int FB, int LANES, int BLOCK, bool RUN_ON, typename HEAD, typename MOVE>
__device__ __forceinline__ void ring_flush(const RingState<HEAD>& st, int ph, bool drain, bool use_list, int np, uint32_t cap, uint32_t ocap, MOVE&& move) {
    static_assert(LANES > 0 && (LANES & (LANES - 1)) == 0 && BLOCK % LANES == 0, "a ring's lanes are a power of two that divides the workgroup");
    const int j = threadIdx.x & (LANES - 1);
    const bool listed = use_list && !drain;
    const int nwalk = listed ? (int)st.nready[ph] : np;
    for (int q = threadIdx.x / LANES; q < nwalk; q += BLOCK / LANES) {
        const int p = listed ? (int)st.ready[q] : q;
        uint32_t f = st.fill[p];
        if (f > cap) f = cap;
        const uint32_t nb = drain ? (f + FB - 1) / FB : f / FB;
        if (nb == 0) continue;
        const uint32_t h = st.head[p], cur = st.cursor[p];
        uint32_t done = 0, wrote = 0;
        for (uint32_t b = 0; b < nb; b++) {
            uint32_t src = h + b * FB;
            if (src >= cap) src -= cap;
            const uint32_t n_here = f - b * FB < (uint32_t)FB ? f - b * FB : FB;
            const uint32_t off = RUN_ON ? done : wrote;
            const bool room = cur + off + FB <= ocap;
            move(p, src, (int64_t)cur + off, n_here, j, room);
            if (room) wrote += n_here;
            done += n_here;
        }
        if (j == 0) {
            uint32_t nh = h + nb * FB;
            while (nh >= cap) nh -= cap;
            st.head[p] = (HEAD)(drain ? 0 : nh);
            st.fill[p] = f - done;
            st.cursor[p] = RUN_ON ? (cur + done < ocap ? cur + done : ocap) : cur + wrote;
        }
    }
}

// One sub-tile of NE entries per lane (bit e of okmask: entry e exists): insert, flush, and as many more rounds as entries are left
// pending (more than cap - FB + 1 new entries of one partition: skew).  try_insert(e) -> the entry found a slot; flush() is the
// kernel's ring_flush(drain = false); stop(nr, pend) -> give up after nr repeated rounds (the kernel's round limit and what it does
// with the entries still pending; called by every thread, so it may hold barriers).
// Round k raises retry[k & 1]; the flag and the list counter of round k + 1 are cleared between the two barriers of round k, when
// nobody reads or raises them.
// The pending entries are a BIT MASK: with two bools the compiler specialised the loop for lanes that have nothing to insert -- a
// second copy of the barriers, executed by the same wave when only some of its lanes hold rows: the partial last sub-tile lost entries.
template <int NE, typename HEAD, typename TRY, typename FLUSH, typename STOP>
__device__ __forceinline__ void ring_rounds(const RingState<HEAD>& st, int& ph, uint32_t okmask, TRY&& try_insert, FLUSH&& flush, STOP&& stop) {
    uint32_t pend = 0;
#pragma unroll
    for (int e = 0; e < NE; e++) if (((okmask >> e) & 1u) && !try_insert(e)) pend |= 1u << e;
    for (int nr = 0;; nr++) {
        if (pend) st.retry[ph] = 1;
        __syncthreads();
        flush();
        if (threadIdx.x == 0) { st.retry[ph ^ 1] = 0; st.nready[ph ^ 1] = 0; }
        __syncthreads();
        const bool again = st.retry[ph] != 0;
        ph ^= 1;
        if (!again || stop(nr, pend)) break;
#pragma unroll
        for (int e = 0; e < NE; e++) if (((pend >> e) & 1u) && try_insert(e)) pend &= ~(1u << e);
    }
}

// ---- a level-2 pass reads the regions level 1 wrote --------------------------------------------------------------------------
// Workgroup g of the in_split that share input partition `pin` takes `per` consecutive regions of it; the concatenation of their
// entries is counted in load UNITS of UNIT entries (a region's last unit may be partial), rstart[] = the prefix of the regions' units.
struct RingRegions {
    int64_t region0;     // the first region: region rj is region0 + rj * rstride
    uint32_t total;      // units in all of them
};
// (rstart: per + 1 words of LDS; region of (partition, region r) = partition * pstride + r * rstride; holds a barrier)
template <int UNIT>
__device__ __forceinline__ RingRegions ring_regions(uint32_t* rstart, const uint32_t* in_counts, int in_regions, int in_split, int64_t pstride, int64_t rstride) {
    const int pin = blockIdx.x / in_split, g = blockIdx.x % in_split;
    const int per_max = (in_regions + in_split - 1) / in_split;
    const int first = g * per_max;
    const int per = first + per_max <= in_regions ? per_max : (in_regions > first ? in_regions - first : 0);
    RingRegions r;
    r.region0 = (int64_t)pin * pstride + (int64_t)first * rstride;
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int rj = 0; rj < per; rj++) { rstart[rj] = run; run += (in_counts[r.region0 + rj * rstride] + UNIT - 1) / UNIT; }
        rstart[per] = run;
    }
    __syncthreads();
    r.total = rstart[per];
    return r;
}
// The region of unit v (< total) and the unit's first entry within it.  A lane visits its units in ascending order: the cursor `reg`
// only moves forward.
template <int UNIT>
__device__ __forceinline__ int ring_region_of(const uint32_t* rstart, int& reg, uint32_t v, uint32_t* e0) {
    int lo = reg;
    while (rstart[lo + 1] <= v) lo++;
    reg = lo;
    *e0 = (uint32_t)UNIT * (v - rstart[lo]);
    return lo;
}

// ---- the side list of the two sample sorts -----------------------------------------------------------------------------------
// Rows that do not travel through the rings (NULL keys, heavy codes) go to a list in HBM whose length is *len: ONE reservation per
// workgroup and sub-tile (one per wave and entry was ~1e6 atomics on one address per 1e9 rows with 0.2 % heavy rows: 14 ms).  A ballot
// per entry slot, the wave's total to cnt[hp], thread 0 reserves, positions from a popcount below the lane.
// cnt[2] (zeroed by the kernel) and base are the workgroup's LDS words for it.  hit(e) -> entry e goes to the list (called by every lane
// for every e); emit(e, pos): store it at list position pos.  Returns the mask of this lane's entries that went.  Holds two barriers.
template <int NE, typename HIT, typename EMIT>
__device__ __forceinline__ uint32_t ring_side_list(uint32_t (&cnt)[2], unsigned long long& base, int& hp, unsigned long long* len, HIT&& hit, EMIT&& emit) {
    uint64_t mm[NE]; uint32_t wtot = 0, mine = 0;
#pragma unroll
    for (int e = 0; e < NE; e++) {
        const bool h = hit(e);
        mine |= (h ? 1u : 0u) << e;
        mm[e] = __ballot(h);
        wtot += (uint32_t)__popcll(mm[e]);
    }
    const int lane = threadIdx.x & 63;
    uint32_t woff = 0;
    if (lane == 0 && wtot) woff = atomicAdd(&cnt[hp], wtot);
    woff = __shfl(woff, 0);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = cnt[hp];
        base = t ? atomicAdd(len, (unsigned long long)t) : 0ULL;
        cnt[hp ^ 1] = 0;
    }
    __syncthreads();
    hp ^= 1;
    if (wtot) {
        const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
        unsigned long long at = base + woff;
#pragma unroll
        for (int e = 0; e < NE; e++) {
            if ((mine >> e) & 1u) emit(e, at + __popcll(mm[e] & lt));
            at += __popcll(mm[e]);
        }
    }
    return mine;
}
