// Sliced layouts ("SELL-64, sorted inside the output window") for the two big sparse products.
//
// Why: with the gathered vector in LDS the products are pure streams of (value, 16-bit index), and
// what kept the segment kernels (k_seg_stream_lds / k_bcsc_lds) at ~63 % of the HBM peak was not the
// stream but the segmented reduction around it -- products through LDS, two workgroup barriers per
// tile, per-segment ptr loads.  Here every lane owns one output (a row of J for J*x, one column
// inside one row-window for J'*y) and adds its products in a register, in index order (= the
// reference's summation order, utils.jl / SparseArrays mul!): no product staging, no barrier inside
// the stream, no ptr array.
//
// Layout, built once per pattern (lsq_sparse.hip: build_sell):
//   * outputs are cut into blocks ("windows") that one 1024-thread workgroup owns:
//       J*x : <= 4096 consecutive rows            (gather vector x: all n entries in LDS; n > 12160: one column window of
//                                                   x at a time, k_sell_rows_wide, block = (row block, window))
//       J'*y: <= 2560 consecutive columns of one <= 16384-row gather window (y[window] in LDS); blocks are placed XCD-aware
//             (lsq_xcd_block: the column blocks of a window behind one L2)
//   * inside a block the outputs are sorted by entry count and grouped 64 at a time (a slice,
//     lane = output); a slice stores max-count L entries per lane, interleaved
//     in pairs:  slot(j, lane) = off + ((j/2)*64 + lane)*2 + (j%2)   -> a lane reads one 16-byte
//     value pair and one 4-byte index pair per step, a wave reads 1 KiB + 256 B contiguous;
//     an ODD slice (round 5: L is no longer rounded up to even) ends with one unpaired entry per lane in a
//     compact group of its own:  slot(L-1, lane) = off + (L/2)*128 + lane  (512 B + 128 B per wave).
//     Sorting makes the padding small (~7 % on the Poisson(10) rows of the C4 workload).
//   * every block is padded to the same number of slices (empty ones at the end), so block b owns slices
//     [b * spw, (b + 1) * spw) and no per-block table has to be read at the head of a launch;
//   * info[slice*64 + lane] = position of the output inside the block | true entry count << 13;
//     slices are stored in "snake" order so that the 16 waves (slice s0+wave, +16, ...) get equal work.
//   * results are dropped into an LDS window at their ORIGINAL position, then one coalesced pass
//     applies the caller's epilogue (J*x) or writes the per-window column partials (J'*y), so the
//     vectors keep the user's order everywhere.
#pragma once

constexpr int LSQ_SELL_POS_BITS = 13;
constexpr unsigned LSQ_SELL_POS_MASK = (1u << LSQ_SELL_POS_BITS) - 1u;   // 0x1fff = "no output" (padding lane)
constexpr int LSQ_SELL_ROWS_MAX = 4096;    // J*x: output rows per block
// J'*y: a block = (gather window of <= 16384 rows of y in LDS: 128 KiB) x (<= 2560 output columns: 20 KiB).  Round 3: twice the
// rows and half the columns of rounds 1-2 (8192 x 5120) -- same number of blocks, but a column's entries inside a window
// double (C4: 7.8 -> 15.6), so the padding of the pair-interleaved slices halves (6.4 % -> 3 %), there are half as many
// per-window partials to write and to combine (C4: 128 -> 64 per column) and half as many lane descriptors to read.
constexpr int LSQ_SELL_CW_AUTO = 6;       // ... chosen by default up to this many (n <= 72960), see lsq_csc_create
constexpr int LSQ_SELL_CW_MAX = 32;       // J*x with n > LSQ_LDS_X_MAX: at most this many column windows of x (k_sell_rows_wide)
constexpr int LSQ_SELL_GROWS_MAX = 16384;
constexpr int LSQ_SELL_CCOLS_MAX = 2560;

struct SellDev {
    const int2 *smeta;            // per slice {entry offset, padded entry count}
    const unsigned *info;         // per (slice, lane)
    const unsigned short *idx16;  // gather index per stored entry
    const double *val;
    int nblocks;
    int spw;                      // slices per block: block b owns slices [b * spw, (b + 1) * spw)
};

// One batch of U value/index pairs of a lane: ALL loads first (each lane has U 20-byte requests in flight), then the sums.
// CLAMP: the slice has fewer than U pairs left; the surplus loads re-read the last pair and their products are dropped by the
// `len` selection, like every padding entry.  (Measured alternatives on C4, J*v launch: skipping the surplus loads behind
// wave-uniform branches 24.4 us against 23.7 us -- the branches split the batch; a fixed 8-wide first batch 24.5 us -- the
// surplus gathers and adds are not free either.)
template <int U>
struct SellBatch {
    double2 a[U];
    unsigned c[U];
};
template <int U, bool CLAMP>
__device__ __forceinline__ void sell_batch_load(SellBatch<U> &B, const double *__restrict__ vp, const unsigned short *__restrict__ ip,
                                                int p0, int np) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int q = CLAMP ? min(p0 + u, np - 1) : p0 + u;
        B.a[u] = *reinterpret_cast<const double2 *>(vp + (size_t)q * 128);
        B.c[u] = *reinterpret_cast<const unsigned *>(ip + (size_t)q * 128);
    }
}
template <int U, bool CLAMP, bool SQ>
__device__ __forceinline__ void sell_batch_sum(SellBatch<U> &B, int p0, int np, int len, const double *xl, double &sum, double &sq) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // every operand is fetched and every sum formed unconditionally; padding is dropped by SELECTION (a
        // conditional add lets the compiler sink the value fetch into an exec-masked block behind a full
        // s_waitcnt vmcnt(0) inside this loop).  The additions happen in entry order.
        const double x0 = xl[B.c[u] & 0xffffu], x1 = xl[B.c[u] >> 16];
        double p0v = B.a[u].x * x0, p1v = B.a[u].y * x1;
        asm volatile("" : "+v"(p0v), "+v"(p1v));   // (the products exist here, whatever the selections below)
        const int j = 2 * (p0 + u);
        // (clamped surplus pairs are never selected: an odd slice has len up to 2 np + 1, so the pair index decides, not len alone)
        const bool pin = !CLAMP || p0 + u < np;
        const bool in0 = pin && j < len, in1 = pin && j + 1 < len;
        const double t0 = sum + p0v;
        sum = in0 ? t0 : sum;
        const double t1 = sum + p1v;
        sum = in1 ? t1 : sum;
        if constexpr (SQ) {
            const double q0 = sq + B.a[u].x * B.a[u].x;
            sq = in0 ? q0 : sq;
            const double q1 = sq + B.a[u].y * B.a[u].y;
            sq = in1 ? q1 : sq;
        }
    }
}

// all products of one lane's output inside one slice (L entries per lane, even and wave-uniform; `len` of them real), added in
// index order.  A slice of the C4 workload holds 4-10 pairs per lane: one batch, one memory round trip (the round-1 loop paid one
// per 4 pairs plus one per leftover pair, in sequence).
// The unpaired last entry of an odd slice (compact group behind the pairs).  vp / ip point at the lane's first pair (off + 2 lane):
// the group's element for this lane sits at off + (L/2)*128 + lane.  Requested with the batches, added last (index order).
struct SellTail {
    double a;
    unsigned short c;
};
__device__ __forceinline__ SellTail sell_tail_load(const double *__restrict__ vp, const unsigned short *__restrict__ ip, int L, int lane) {
    SellTail t;
    const long long o = (long long)(L >> 1) * 128 - lane;
    t.a = vp[o];
    t.c = ip[o];
    return t;
}
template <bool SQ>
__device__ __forceinline__ void sell_tail_sum(const SellTail &t, int L, int len, const double *xl, double &sum, double &sq) {
    double p = t.a * xl[t.c];
    asm volatile("" : "+v"(p));
    const bool in = L - 1 < len;
    const double s1 = sum + p;
    sum = in ? s1 : sum;
    if constexpr (SQ) {
        const double q1 = sq + t.a * t.a;
        sq = in ? q1 : sq;
    }
}
template <bool SQ, bool TAIL = true>
__device__ __forceinline__ void sell_lane_sum_from(const double *__restrict__ vp, const unsigned short *__restrict__ ip, int p0, int L,
                                                   int len, const double *xl, double &sum, double &sq, int lane) {
    const int np = L >> 1;
    SellTail tail;
    tail.a = 0.0;
    tail.c = 0;
    if (TAIL && (L & 1)) tail = sell_tail_load(vp, ip, L, lane);      // (wave-uniform; in flight with the batches)
    for (; p0 + 8 <= np; p0 += 8) {
        SellBatch<8> B;
        sell_batch_load<8, false>(B, vp, ip, p0, np);
        sell_batch_sum<8, false, SQ>(B, p0, np, len, xl, sum, sq);
    }
    const int rem = np - p0;
    if (rem > 4) {
        SellBatch<8> B;
        sell_batch_load<8, true>(B, vp, ip, p0, np);
        sell_batch_sum<8, true, SQ>(B, p0, np, len, xl, sum, sq);
    } else if (rem > 2) {
        SellBatch<4> B;
        sell_batch_load<4, true>(B, vp, ip, p0, np);
        sell_batch_sum<4, true, SQ>(B, p0, np, len, xl, sum, sq);
    } else if (rem > 0) {
        SellBatch<2> B;
        sell_batch_load<2, true>(B, vp, ip, p0, np);
        sell_batch_sum<2, true, SQ>(B, p0, np, len, xl, sum, sq);
    }
    if (TAIL && (L & 1)) sell_tail_sum<SQ>(tail, L, len, xl, sum, sq);
}

template <bool SQ>
__device__ __forceinline__ void sell_lane_sum(const double *__restrict__ vp, const unsigned short *__restrict__ ip, int L, int len,
                                              const double *xl, double &sum, double &sq, int lane) {
    sell_lane_sum_from<SQ>(vp, ip, 0, L, len, xl, sum, sq, lane);
}

// ---- the head of a streaming launch --------------------------------------------------------------------------------------
// The gather vector goes global -> LDS by LDS-DMA (gfx950: global_load_lds_dwordx4, no register destination), so a thread
// holds no staging array and the FIRST slice of every wave can have its value / index batch requested while the vector is
// still on its way: one wait (vmcnt(0) in front of the barrier) retires both.  With the vector staged through registers the
// same prefetch spilled (12-16 doubles of staging + 40 registers of batch per lane at the 128-register cap of a 1024-thread
// workgroup).
// The LDS image is lane-linear: 16-byte chunk q * 1024 + tid lands at lds + 2 * (q * 1024 + tid) -- the DMA's destination is
// "wave-uniform base + lane * 16", the base taken from the first active lane, and the active lanes of a wave are a prefix.
// `src` must be 16-byte aligned (sell_stage_dma_ok: workgroup-uniform; otherwise the caller stages through registers), `lds`
// too.  An odd count leaves its last double to a plain load of thread 0, written by sell_stage_tail_write in front of the
// barrier.  A wave must not END with a DMA outstanding (its LDS may belong to the next workgroup by the time the data lands):
// every early return behind a sell_stage_dma goes through sell_stage_wait.
// Every chunk sits behind a per-lane predicate, i.e. in a block of its own that a wave may skip.  A load whose result the compiler
// still counts as unused on SOME path into these blocks (the register-staging alternative beside them, say) makes it wait
// vmcnt(0) in front of every chunk, which at run time drains the chunk before it: the alternative path ends in sell_stage_wait
// for that reason.  What a kernel requests BEFORE the DMA and uses behind it (the first slice's descriptor) is waited for by
// count and leaves the DMA in flight.
struct SellStageTail {
    double v;
    int at;       // LDS index of the unpaired last element, or -1
};
__device__ __forceinline__ bool sell_stage_dma_ok(const double *src) { return ((unsigned long long)src & 15ull) == 0ull; }
// s_waitcnt vmcnt(0) as the builtin (gfx9 encoding: expcnt and lgkmcnt left at their maxima), which the compiler's own counter
// bookkeeping sees -- an inline-asm wait it does not
__device__ __forceinline__ void sell_stage_wait() { __builtin_amdgcn_s_waitcnt(0x0F70); }
template <int NQ>      // chunks per thread: NQ * 1024 * 2 >= count
__device__ __forceinline__ SellStageTail sell_stage_dma(const double *__restrict__ src, double *lds, int count, int tid) {
    typedef const __attribute__((address_space(1))) void *gptr_t;
    typedef __attribute__((address_space(3))) void *lptr_t;
    const int nch = count >> 1;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int ch = q * LSQ_BIG_NT + tid;
        if (ch < nch) __builtin_amdgcn_global_load_lds((gptr_t)(src + 2 * ch), (lptr_t)(lds + 2 * ch), 16, 0, 0);
    }
    SellStageTail t;
    t.v = 0.0;
    t.at = -1;
    if ((count & 1) && tid == 0) {
        t.v = src[count - 1];
        t.at = count - 1;
    }
    return t;
}
__device__ __forceinline__ void sell_stage_tail_write(const SellStageTail &t, double *lds) {
    if (t.at >= 0) lds[t.at] = t.v;
}

// The first batch of a slice, requested ahead of the barrier that hands the gather vector over (sell_head_load) and added
// behind it (sell_lane_sum_head): the same operands, the same additions in the same order as sell_lane_sum -- the first batch
// is loaded and selected with the clamped forms, which are the identity where the slice has 8 pairs or more.
// (Named members, not arrays: the head lives across the barrier and several branches, and an array member there kept the
//  whole struct in scratch memory; the batch itself is a local SellBatch on either side, as everywhere.)
struct SellHead {
    double2 a0, a1, a2, a3, a4, a5, a6, a7;
    unsigned c0, c1, c2, c3, c4, c5, c6, c7;
    double ta;
    unsigned tc;
};
template <int U>
__device__ __forceinline__ void sell_head_put(SellHead &H, const SellBatch<U> &B) {
    static_assert(U == 2 || U == 4 || U == 8, "head batch");
    H.a0 = B.a[0]; H.c0 = B.c[0];
    H.a1 = B.a[1]; H.c1 = B.c[1];
    if constexpr (U >= 4) {
        H.a2 = B.a[2]; H.c2 = B.c[2];
        H.a3 = B.a[3]; H.c3 = B.c[3];
    }
    if constexpr (U >= 8) {
        H.a4 = B.a[4]; H.c4 = B.c[4];
        H.a5 = B.a[5]; H.c5 = B.c[5];
        H.a6 = B.a[6]; H.c6 = B.c[6];
        H.a7 = B.a[7]; H.c7 = B.c[7];
    }
}
template <int U>
__device__ __forceinline__ void sell_head_get(const SellHead &H, SellBatch<U> &B) {
    B.a[0] = H.a0; B.c[0] = H.c0;
    B.a[1] = H.a1; B.c[1] = H.c1;
    if constexpr (U >= 4) {
        B.a[2] = H.a2; B.c[2] = H.c2;
        B.a[3] = H.a3; B.c[3] = H.c3;
    }
    if constexpr (U >= 8) {
        B.a[4] = H.a4; B.c[4] = H.c4;
        B.a[5] = H.a5; B.c[5] = H.c5;
        B.a[6] = H.a6; B.c[6] = H.c6;
        B.a[7] = H.a7; B.c[7] = H.c7;
    }
}
// `off` and `L` are SCALARS here (the caller passes them through readfirstlane): every request is "scalar base + the lane's
// offset", one lane offset for the eight value requests and one for the eight index requests -- with per-lane 64-bit addresses
// (what sell_batch_load forms from a descriptor in vector registers) the sixteen addresses alone cost 32 registers.
// ONE form of the request whatever the slice's length (a short slice re-reads its last pair: lines it has requested anyway).
// Requests of 2, 4 or 8 pairs behind branches, as in sell_lane_sum_from, end in stores to different members of H that the
// compiler merges into one store through a computed address -- and H then lives in scratch memory.
__device__ __forceinline__ void sell_head_load(SellHead &H, const double *__restrict__ val, const unsigned short *__restrict__ idx,
                                               int off, int L, int lane) {
    typedef const __attribute__((address_space(1))) char *gchar_t;
    typedef double __attribute__((ext_vector_type(2))) gd2_t;
    const int np = L >> 1;
    // (byte offsets of the lane as 32-bit values: the "scalar base + 32-bit lane offset" form of a global load)
    unsigned vo = 16u * (unsigned)lane, io = 4u * (unsigned)lane;
    asm volatile("" : "+v"(vo), "+v"(io));      // (formed HERE: hoisted out of this block as 64-bit values they cost an add per request)
    const char *vb = reinterpret_cast<const char *>(val + off);
    const char *ib = reinterpret_cast<const char *>(idx + off);
    H.ta = 0.0;
    H.tc = 0u;
    if (L & 1) {
        unsigned long long vt = (unsigned long long)(vb + (size_t)np * 1024), it = (unsigned long long)(ib + (size_t)np * 256);
        asm volatile("" : "+s"(vt), "+s"(it));
        H.ta = *(const __attribute__((address_space(1))) double *)((gchar_t)vt + (vo >> 1));
        // (the lane's 16-bit index inside an aligned 32-bit word, picked behind the barrier: a 16-bit load is widened where it
        //  is issued, which is a use -- and a wait -- in front of the barrier)
        H.tc = *(const __attribute__((address_space(1))) unsigned *)((gchar_t)it + ((io >> 1) & ~3u));
    }
    if (np > 0) {
        SellBatch<8> B;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t q = (size_t)min(u, np - 1);
            // (scalar bases, pinned: not folded into a per-lane 64-bit address.  The pin goes through an integer, so the pointer
            //  is rebuilt as a GLOBAL one -- a generic pointer would make these flat loads.)
            unsigned long long vq = (unsigned long long)(vb + q * 1024), iq = (unsigned long long)(ib + q * 256);
            asm volatile("" : "+s"(vq), "+s"(iq));
            const gd2_t v = *(const __attribute__((address_space(1))) gd2_t *)((gchar_t)vq + vo);
            B.a[u].x = v.x;
            B.a[u].y = v.y;
            B.c[u] = *(const __attribute__((address_space(1))) unsigned *)((gchar_t)iq + io);
        }
        sell_head_put<8>(H, B);
    }
}
template <int U, bool SQ>
__device__ __forceinline__ void sell_head_sum_n(const SellHead &H, int np, int len, const double *xl, double &sum, double &sq) {
    SellBatch<U> B;
    sell_head_get<U>(H, B);
    sell_batch_sum<U, true, SQ>(B, 0, np, len, xl, sum, sq);
}
template <bool SQ>
__device__ __forceinline__ void sell_lane_sum_head(const SellHead &H, const double *__restrict__ vp, const unsigned short *__restrict__ ip,
                                                   int L, int len, const double *xl, double &sum, double &sq, int lane) {
    const int np = L >> 1;
    if (np > 4) sell_head_sum_n<8, SQ>(H, np, len, xl, sum, sq);
    else if (np > 2) sell_head_sum_n<4, SQ>(H, np, len, xl, sum, sq);
    else if (np > 0) sell_head_sum_n<2, SQ>(H, np, len, xl, sum, sq);
    if (np > 8) sell_lane_sum_from<SQ, false>(vp, ip, 8, L, len, xl, sum, sq, lane);
    if (L & 1) {
        SellTail t;
        t.a = H.ta;
        t.c = (unsigned short)(H.tc >> (16 * (lane & 1)));
        sell_tail_sum<SQ>(t, L, len, xl, sum, sq);
    }
}

// The slices of one wave (s0 + wave, + 16, ...), with the next slice's descriptor requested before the current slice's stream.
//   `out(pos, sum, sq)` stores a lane's result.
// Contains the workgroup barrier that separates staging the gather vector from the first gather: the first slice's descriptor
// AND its first batch are requested before it (the value addresses need only the slice's wave-uniform {offset, L}; the per-lane
// word `info` is first used in the sums, behind the barrier -- with a DMA in flight the compiler waits for everything at the
// first use of a vector load's result).  `before_barrier()` runs between those requests and the barrier (the staged vector's
// odd tail, the wait for the DMA).  `stop` (workgroup-uniform) ends the launch behind the barrier: the `done` flag of a launch
// queued behind a finished solve is requested with everything else at the head -- one latency, not two in a row -- and acted
// on here, where nothing is outstanding any more; the function then returns true and the caller returns.
// `first` (if have_first): the descriptor of slice s0 + wave, requested by the caller AHEAD of the DMA -- a vector load requested behind
// it could only be waited for together with it.
// (Requesting TWO slices per wave up front made the J*v launch slower, 29.5 us against 23.7 us: the
// stream is not short of requests in flight, a CU's miss queue is already full with 16 waves x 5-8 KB.)
struct SellNoBeforeBarrier {
    __device__ __forceinline__ void operator()() const {}
};
struct SellSliceRef {
    int2 sm;        // {entry offset, padded entry count}
    unsigned inf;   // position | true count << 13
};
__device__ __forceinline__ SellSliceRef sell_slice_ref(const SellDev &S, int s, int s1, int lane) {
    SellSliceRef r;
    r.sm = make_int2(0, 0);
    r.inf = LSQ_SELL_POS_MASK;
    if (s < s1) {
        r.sm = S.smeta[__builtin_amdgcn_readfirstlane(s)];
        r.inf = S.info[(size_t)s * 64 + lane];
    }
    return r;
}
//   `hook` (optional) also sees a lane's sum at its SLICE-ORDER index s * 64 + lane (what k_sell_rows_pair reads and writes):
//   pre(pidx) is requested before the slice's stream, post(pidx, sum, pre) follows the lane's result.
struct SellNoSliceHook {
    __device__ __forceinline__ double pre(size_t) const { return 0.0; }
    __device__ __forceinline__ void post(size_t, double, double) const {}
};
template <bool SQ, class Out, class Hook = SellNoSliceHook, class Before = SellNoBeforeBarrier>
__device__ __forceinline__ bool sell_wave_slices(const SellDev &S, int s0, int s1, int wv, int lane, const double *xl, Out out,
                                                 Hook hook = Hook(), Before before_barrier = Before(), int stop = 0,
                                                 bool have_first = false, SellSliceRef first = SellSliceRef()) {
    constexpr int NW = LSQ_BIG_NT / 64;
    int s = s0 + wv;
    SellSliceRef A;
    A.sm = make_int2(0, 0);
    A.inf = LSQ_SELL_POS_MASK;
    if (!have_first) A = sell_slice_ref(S, s, s1, lane);
    SellHead H;
    double hp0 = 0.0;
    // the first slice's {offset, L} as SCALARS: its eight value and eight index requests then share one lane offset
    // (`info` of a caller's descriptor is not touched before the barrier: merging it here would be a use)
    const int2 smv = have_first ? first.sm : A.sm;
    const int2 sm0 = make_int2(__builtin_amdgcn_readfirstlane(smv.x), __builtin_amdgcn_readfirstlane(smv.y));
    if (s < s1) {                                           // (wave-uniform)
        sell_head_load(H, S.val, S.idx16, sm0.x, sm0.y, lane);
        hp0 = hook.pre((size_t)s * 64 + lane);
    }
    before_barrier();
    __syncthreads();
    // (workgroup-uniform: the caller's `done` flag, see there.  The empty asm pins the flag's first USE here: the compiler otherwise
    //  turns it into a branch condition where it was loaded, and waits for it -- and with it for the DMA -- at the head.)
    asm volatile("" : "+v"(stop));
    if (stop) return true;
    if (s < s1) {                                           // the first slice: its first batch is already here
        SellSliceRef a;
        a.sm = sm0;
        unsigned inf1 = first.inf;
        asm volatile("" : "+v"(inf1));      // (its first use is HERE, behind the barrier: the compiler otherwise copies it where `first` is chosen)
        a.inf = have_first ? inf1 : A.inf;
        A = sell_slice_ref(S, s + NW, s1, lane);
        const size_t oa = (size_t)a.sm.x + lane * 2;
        const unsigned pos = a.inf & LSQ_SELL_POS_MASK;
        const size_t pidx = (size_t)s * 64 + lane;
        double sum = 0.0, sq = 0.0;
        sell_lane_sum_head<SQ>(H, S.val + oa, S.idx16 + oa, a.sm.y, (int)(a.inf >> LSQ_SELL_POS_BITS), xl, sum, sq, lane);
        if (pos != LSQ_SELL_POS_MASK) {
            out(pos, sum, sq);
            hook.post(pidx, sum, hp0);
        }
        s += NW;
    }
    for (; s < s1; s += NW) {
        const SellSliceRef a = A;
        A = sell_slice_ref(S, s + NW, s1, lane);
        const size_t oa = (size_t)a.sm.x + lane * 2;
        const unsigned pos = a.inf & LSQ_SELL_POS_MASK;
        const size_t pidx = (size_t)s * 64 + lane;
        const double hp = hook.pre(pidx);                   // (coalesced; in flight during the stream)
        double sum = 0.0, sq = 0.0;
        sell_lane_sum<SQ>(S.val + oa, S.idx16 + oa, a.sm.y, (int)(a.inf >> LSQ_SELL_POS_BITS), xl, sum, sq, lane);
        if (pos != LSQ_SELL_POS_MASK) {
            out(pos, sum, sq);
            hook.post(pidx, sum, hp);
        }
    }
    return false;
}
// an epilogue that wants its rows in slice order as well (has_slice_out): slice_pre / slice_post, see sell_wave_slices
template <class Epi>
struct SellEpiSliceHook {
    const Epi &epi;
    __device__ __forceinline__ double pre(size_t pidx) const { return epi.slice_pre(pidx); }
    __device__ __forceinline__ void post(size_t pidx, double sum, double p) const { epi.slice_post(pidx, sum, p); }
};

// ---- J*x: dot of every row with x, then the epilogue on (row, dot) in row order ----------------
// xscale (or null): the matrix is the stored values times diag(xscale) -- a COLUMN-SCALED Jacobian J = V diag(s) whose scaled
// entries are never materialised (lsq_mat::d_colscale): the gather vector is staged as s .* x, the stream is V's.
template <class Epi>
__global__ void __launch_bounds__(LSQ_BIG_NT) k_sell_rows(SellDev S, int wrows, int m, const double *__restrict__ x,
                                                          const double *__restrict__ xscale, int nx, int nxpad, Epi epi) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double sh[LSQ_BIG_NT / 64];
    double *xl = smem;            // nxpad doubles
    double *yw = smem + nxpad;    // LSQ_SELL_ROWS_MAX doubles
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the gather vector is fetched FIRST, together with the `done` flag of a finished solve and the epilogue's scalars:
    // one memory latency at the head of the kernel instead of three in a row
    constexpr int XR = (LSQ_LDS_X_MAX + LSQ_BIG_NT - 1) / LSQ_BIG_NT;
    SellStageTail xtail;
    xtail.v = 0.0;
    xtail.at = -1;
    const bool dma = !xscale && sell_stage_dma_ok(x);      // (workgroup-uniform)
    // (the first slice's descriptor: requested ahead of the DMA, see sell_wave_slices)
    const SellSliceRef ref0 = sell_slice_ref(S, (int)blockIdx.x * S.spw + wv, (int)blockIdx.x < S.nblocks ? ((int)blockIdx.x + 1) * S.spw : 0, lane);
    int dflag;
    if (dma) {
        // an unscaled vector goes straight to LDS; the first slice's batch follows it inside sell_wave_slices, one wait for both
        xtail = sell_stage_dma<(XR + 1) / 2>(x, xl, nx, tid);
        dflag = epi.done ? *epi.done : 0;
        if constexpr (EpiHasBlockPrepare<Epi>::value) epi.block_prepare();
        if constexpr (EpiHasPrepare<Epi>::value) epi.prepare();
    } else {
        double xr[XR];
#pragma unroll
        for (int q = 0; q < XR; ++q) xr[q] = x[min(tid + q * LSQ_BIG_NT, nx - 1)];
        if (xscale) {   // (wave-uniform; the factors travel with the gather vector: still one latency at the head)
            double sr[XR];
#pragma unroll
            for (int q = 0; q < XR; ++q) sr[q] = xscale[min(tid + q * LSQ_BIG_NT, nx - 1)];
#pragma unroll
            for (int q = 0; q < XR; ++q) xr[q] *= sr[q];
        }
        dflag = epi.done ? *epi.done : 0;

        if constexpr (EpiHasBlockPrepare<Epi>::value) epi.block_prepare();
        if constexpr (EpiHasPrepare<Epi>::value) epi.prepare();
#pragma unroll
        for (int q = 0; q < XR; ++q)
            if (tid + q * LSQ_BIG_NT < nx) xl[tid + q * LSQ_BIG_NT] = xr[q];
        sell_stage_wait();      // (nothing left that counts as pending: see sell_stage_dma)
    }
    // launches queued behind a finished solve stop behind the first barrier (sell_wave_slices: `stop`); without a block, here
    if ((int)blockIdx.x >= S.nblocks) {
        sell_stage_wait();
        int d = dflag;
        asm volatile("" : "+v"(d));      // (the flag's use stays inside this branch)
        if (d) return;
    }
    bool pending = dma;      // a DMA is outstanding: waited for in front of the first barrier
    constexpr int Q = LSQ_SELL_ROWS_MAX / LSQ_BIG_NT;
    double racc = 0.0;
    for (int w = blockIdx.x; w < S.nblocks; w += gridDim.x) {
        const int base = w * wrows, rows = min(wrows, m - base);
        const int s0 = w * S.spw, s1 = s0 + S.spw;
        double pre[Q];
        if constexpr (EpiHasPre<Epi>::value) {   // epilogue inputs of this window: in flight during the stream
#pragma unroll
            for (int q = 0; q < Q; ++q) pre[q] = epi.pre(base + min(tid + q * LSQ_BIG_NT, rows - 1));
        }
        // (the barrier inside: x staged / the previous window's epilogue is done with yw)
        auto staged = [&]() {      // (the odd last element of a DMA-staged x; nothing of the DMA is outstanding at the barrier)
            sell_stage_tail_write(xtail, xl);
            if (pending) sell_stage_wait();
        };
        bool stopped;
        if constexpr (EpiHasSliceOut<Epi>::value)
            stopped = sell_wave_slices<false>(S, s0, s1, wv, lane, xl, [&](unsigned pos, double sum, double) { yw[pos] = sum; },
                                              SellEpiSliceHook<Epi>{epi}, staged, dflag, w == (int)blockIdx.x, ref0);
        else
            stopped = sell_wave_slices<false>(S, s0, s1, wv, lane, xl, [&](unsigned pos, double sum, double) { yw[pos] = sum; },
                                              SellNoSliceHook(), staged, dflag, w == (int)blockIdx.x, ref0);
        if (stopped) return;
        xtail.at = -1;
        pending = false;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = tid + q * LSQ_BIG_NT;
            if (i < rows) {
                if constexpr (EpiHasPre<Epi>::value) epi.seg_pre(base + i, yw[i], pre[q], racc);
                else epi.seg(base + i, yw[i], racc);
            }
        }
        // (nothing of this block counts as pending at the loop's head: the compiler merges what is pending there with what is
        //  pending at the launch's head, and would wait for the DMA before the first request.  The barriers behind the loop wait
        //  for these stores anyway.)
        sell_stage_wait();
    }
    // side work (e.g. damped rows) is laid out for LSQ_NT-thread blocks
    for (int e = blockIdx.x; e < epi.extra_blocks; e += gridDim.x)
        if (tid < LSQ_NT) epi.extra(e, racc);
    finish_block_nt<LSQ_BIG_NT>(epi, racc, sh);
}

// ---- TWO products with the same stored values in ONE pass: rows of V*(s .* xa) and of V*xb --------------------------
// The tail of an LM iteration on a model r(x) = V phi(x) - b with the column-scaled Jacobian J = V diag(s) streams V twice:
// the predicted residual |J dx - f|^2 (levenberg_marquardt.jl:114-117) and the trial residual f!(x_trial) = V phi(x_trial) - b
// with its sum of squares (:107, :111) -- 2 x 107 MB at C4 for 16 MB of vectors.  Here every (value, index) pair is loaded
// once and multiplied into both gather vectors.  Both vectors must be resident in LDS (2 x 8n bytes: n <= 10200 with the
// 160 KB of a CU), which leaves no room for the output window of k_sell_rows: a lane applies the epilogue to its row itself
// (f[i], b[i] requested at the head of the slice, the trial residual stored straight from the lane -- 8-byte accesses inside
// the block's 32 KB window, merged in L2).  A row's two sums are formed left to right by one lane, as everywhere: the bits
// of J dx and of V phi(x_trial) are those of the two separate launches; the two sums of squares are added per lane in slice
// order, then wave tree / 16 waves / blocks in index order (deterministic; another association than the row-order pass of
// the separate launches, i.e. equal to it to round-off).
template <int U, bool CLAMP>
__device__ __forceinline__ void sell_batch_sum2(SellBatch<U> &B, int p0, int np, int len, const double *xa, const double *xb,
                                                double &sa, double &sb) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned i0 = B.c[u] & 0xffffu, i1 = B.c[u] >> 16;
        double a0 = B.a[u].x * xa[i0], a1 = B.a[u].y * xa[i1], b0 = B.a[u].x * xb[i0], b1 = B.a[u].y * xb[i1];
        asm volatile("" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1));   // (the products exist here: see sell_batch_sum)
        const int j = 2 * (p0 + u);
        const bool pin = !CLAMP || p0 + u < np;
        const bool in0 = pin && j < len, in1 = pin && j + 1 < len;
        const double ta0 = sa + a0;
        sa = in0 ? ta0 : sa;
        const double ta1 = sa + a1;
        sa = in1 ? ta1 : sa;
        const double tb0 = sb + b0;
        sb = in0 ? tb0 : sb;
        const double tb1 = sb + b1;
        sb = in1 ? tb1 : sb;
    }
}
__device__ __forceinline__ void sell_lane_sum2(const double *__restrict__ vp, const unsigned short *__restrict__ ip, int L, int len,
                                               const double *xa, const double *xb, double &sa, double &sb, int lane) {
    const int np = L >> 1;
    int p0 = 0;
    SellTail tail;
    tail.a = 0.0;
    tail.c = 0;
    if (L & 1) tail = sell_tail_load(vp, ip, L, lane);      // (the unpaired last entry of an odd slice)
    for (; p0 + 8 <= np; p0 += 8) {
        SellBatch<8> B;
        sell_batch_load<8, false>(B, vp, ip, p0, np);
        sell_batch_sum2<8, false>(B, p0, np, len, xa, xb, sa, sb);
    }
    const int rem = np - p0;
    if (rem > 4) {
        SellBatch<8> B;
        sell_batch_load<8, true>(B, vp, ip, p0, np);
        sell_batch_sum2<8, true>(B, p0, np, len, xa, xb, sa, sb);
    } else if (rem > 2) {
        SellBatch<4> B;
        sell_batch_load<4, true>(B, vp, ip, p0, np);
        sell_batch_sum2<4, true>(B, p0, np, len, xa, xb, sa, sb);
    } else if (rem > 0) {
        SellBatch<2> B;
        sell_batch_load<2, true>(B, vp, ip, p0, np);
        sell_batch_sum2<2, true>(B, p0, np, len, xa, xb, sa, sb);
    }
    if (L & 1) {
        double pa = tail.a * xa[tail.c], pb = tail.a * xb[tail.c];
        asm volatile("" : "+v"(pa), "+v"(pb));
        const bool in = L - 1 < len;
        const double ta = sa + pa, tb = sb + pb;
        sa = in ? ta : sa;
        sb = in ? tb : sb;
    }
}
constexpr int LSQ_PAIR_X_MAX = 10200;      // doubles per gather vector: 2 x 10200 x 8 B + the kernel's static LDS (~140 B) <= 160 KB
struct SellPairEpi {
    const int *done;            // skip flag of a launch queued behind an undecided LSMR solve (LsmrTail), or null
    // the two m-vectors the epilogue reads come in SLICE ORDER (element s * 64 + lane = the row that lane of slice s owns;
    // k_sell_perm_rows): a lane's 8-byte access to its row's own position is one cache line per lane -- 64 line requests per
    // wave instruction, as many as the whole value + index stream of the slice; measured 42.7 us with f, b and the output all
    // in row order, 35.6 us with f and b in slice order, 30.8 us with the output in slice order too (profiles/r04)
    const double *fa;           // f (current residual), slice order:  ra = (V (s .* xa))_i - fa_i,  sum ra^2 -> *slot_a
    const double *fb;           // b (model constant), slice order:    rb = (V xb)_i - fb_i,  sum rb^2 -> *slot_b
    double *out_b;              // rb in row order (what the gather of J'f and the caller read)
    double *out_b_perm;         // rb in slice order (the next iteration's fa if the step is accepted)
    double *part_a, *part_b;    // block partials (gridDim.x each)
    unsigned *counter;          // ticket slot of grid_reduce
    double *slot_a, *slot_b;
    LsqSlotPublish pub;         // the iteration's scalars -> host once both sums are final
    // LM's acceptance test AND its convergence test taken on the device as well (levenberg_marquardt.jl:118-122 and utils.jl:7-31,
    // the host's own expressions on the same doubles): *gate = 0 if the step will be accepted and the loop goes on, 1 if not --
    // the skip word of the NEXT iteration's gradient pass, which is queued behind this kernel before the host has seen the
    // scalars (null: no such pass is queued).  A pass behind a converging step would run for a Jacobian nobody forms.
    int *gate;
    double ssr, min_quality;
    double *slot_gate;          // "the pass runs" as a scalar (1.0 / 0.0) among the published ones: the host adopts the queued
                                // pass only if it ran AND the host's own decision is "accepted, not converged"
    const double *slot_dx, *slot_gr;    // max |dx| and max |gradient| of this iteration (final before this kernel starts)
    double xtol, ftol, gtol;
};
// dst[s * 64 + lane] = src[row owned by lane of slice s] (0 for lanes without a row): an m-vector in slice order
template <int = 0>
__global__ void __launch_bounds__(LSQ_NT) k_sell_perm_rows(SellDev S, int wrows, int nslices, const double *__restrict__ src,
                                                           double *__restrict__ dst) {
    for (long long i = blockIdx.x * (long long)LSQ_NT + threadIdx.x; i < (long long)nslices * 64; i += (long long)gridDim.x * LSQ_NT) {
        const unsigned inf = S.info[i];
        const unsigned pos = inf & LSQ_SELL_POS_MASK;
        const int w = (int)(i >> 6) / S.spw;
        dst[i] = pos != LSQ_SELL_POS_MASK ? src[(size_t)w * wrows + pos] : 0.0;
    }
}
template <int = 0>     // (a template so that the header can be included by several translation units)
__global__ void __launch_bounds__(LSQ_BIG_NT) k_sell_rows_pair(SellDev S, int wrows, int m, const double *__restrict__ xa,
                                                               const double *__restrict__ sa_scale, const double *__restrict__ xb,
                                                               int nx, int nxpad, SellPairEpi e) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double sh[LSQ_BIG_NT / 64];
    double *la = smem, *lb = smem + nxpad;
    constexpr int NW = LSQ_BIG_NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int XR = (LSQ_PAIR_X_MAX + LSQ_BIG_NT - 1) / LSQ_BIG_NT;
    {   // both gather vectors and the factors: one memory latency at the head
        double ra[XR], rs[XR], rb[XR];
#pragma unroll
        for (int q = 0; q < XR; ++q) {
            const int i = min(tid + q * LSQ_BIG_NT, nx - 1);
            ra[q] = xa[i];
            rs[q] = sa_scale ? sa_scale[i] : 1.0;
            rb[q] = xb[i];
        }
        const int dflag = e.done ? *e.done : 0;
#pragma unroll
        for (int q = 0; q < XR; ++q)
            if (tid + q * LSQ_BIG_NT < nx) {
                la[tid + q * LSQ_BIG_NT] = ra[q] * rs[q];
                lb[tid + q * LSQ_BIG_NT] = rb[q];
            }
        if (dflag) return;
    }
    // The trial residual goes out twice: in slice order (coalesced, straight from the lane) and in ROW order.  A lane's 8-byte store
    // to "its" row is one cache line per lane (round 4: 2.06x the write traffic this kernel owes, 38.3 us instead of 30.8 with
    // everything in slice order).  Round 5: a lane keeps the residuals of its (at most G) slices in registers; when the block's
    // stream is over the gather vectors are dead, so their LDS becomes the output window that did not fit beside them -- results
    // dropped at their row positions, one coalesced pass to memory.  (A workgroup that owns several blocks re-stages the gather
    // vectors from the cache for the next one; C4: one block per workgroup.)
    constexpr int G = LSQ_SELL_ROWS_MAX / 64 / NW;      // slices per wave and block
    double acc_a = 0.0, acc_b = 0.0;
    for (int w = blockIdx.x; w < S.nblocks; w += gridDim.x) {
        const int base = w * wrows, rows = min(wrows, m - base);
        const int s0 = w * S.spw, s1 = s0 + S.spw;
        if (w != (int)blockIdx.x) {           // the output pass of the previous block used the window: stage the gather vectors again
            __syncthreads();
            for (int i = tid; i < nx; i += LSQ_BIG_NT) {
                la[i] = xa[i] * (sa_scale ? sa_scale[i] : 1.0);
                lb[i] = xb[i];
            }
        }
        int s = s0 + wv;
        SellSliceRef A = sell_slice_ref(S, s, s1, lane);
        __syncthreads();                      // the gather vectors are staged -- nothing else is shared
        double keep[G];
        unsigned kpos[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            kpos[g] = LSQ_SELL_POS_MASK;
            keep[g] = 0.0;
            if (s < s1) {                     // (wave-uniform)
                const SellSliceRef a = A;
                A = sell_slice_ref(S, s + NW, s1, lane);
                const unsigned pos = a.inf & LSQ_SELL_POS_MASK;
                const bool valid = pos != LSQ_SELL_POS_MASK;
                const size_t pidx = (size_t)s * 64 + lane;
                const double fa = e.fa[pidx], fb = e.fb[pidx];        // (coalesced; in flight during the stream)
                const size_t oa = (size_t)a.sm.x + lane * 2;
                double sum_a = 0.0, sum_b = 0.0;
                sell_lane_sum2(S.val + oa, S.idx16 + oa, a.sm.y, (int)(a.inf >> LSQ_SELL_POS_BITS), la, lb, sum_a, sum_b, lane);
                if (valid) {
                    const double r_a = sum_a - fa, r_b = sum_b - fb;
                    e.out_b_perm[pidx] = r_b;
                    keep[g] = r_b;
                    kpos[g] = pos;
                    acc_a += r_a * r_a;
                    acc_b += r_b * r_b;
                }
                s += NW;
            }
        }
        __syncthreads();                      // every gather of this block is done: the vectors' LDS is free
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (kpos[g] != LSQ_SELL_POS_MASK) smem[kpos[g]] = keep[g];
        __syncthreads();
        for (int i = tid; i < rows; i += LSQ_BIG_NT) e.out_b[base + i] = smem[i];
    }
    const double ba = block_sum<LSQ_BIG_NT>(acc_a, sh);
    const double bb = block_sum<LSQ_BIG_NT>(acc_b, sh);
    if (tid == 0) __hip_atomic_store(&e.part_b[blockIdx.x], bb, RLX_AGENT);   // (drained with part_a's store inside grid_reduce)
    double total_a = 0.0;
    const bool last = grid_reduce<LSQ_BIG_NT>(ba, e.part_a, e.counter, gridDim.x, sh, [&](double t) { total_a = t; });
    if (!last) return;
    double pb = 0.0;
    for (int i = tid; i < (int)gridDim.x; i += LSQ_BIG_NT) pb += __hip_atomic_load(&e.part_b[i], RLX_AGENT);
    const double total_b = block_sum<LSQ_BIG_NT>(pb, sh);
    if (tid == 0) {
        *e.slot_a = total_a;
        *e.slot_b = total_b;
        if (e.gate) {
            const double pred_red = fabs(e.ssr - total_a);
            const double rho = pred_red > 0 ? (e.ssr - total_b) / pred_red : 0.0;
            const bool acc = rho > e.min_quality;
            // (the if/elseif chain of the host's assess(): which flag fires does not matter here, only whether one does)
            const bool conv = (acc && fabs(total_b - e.ssr) <= e.ftol * (fabs(e.ssr) + e.ftol)) || *e.slot_dx <= e.xtol ||
                              *e.slot_gr <= e.gtol;
            const bool go = acc && !conv;
            *e.gate = go ? 0 : 1;
            *e.slot_gate = go ? 1.0 : 0.0;
        }
        if (e.pub.count > 0) {
            for (int i = 0; i < e.pub.count; ++i) {
                const double *src = e.pub.src + i;
                const double v = src == e.slot_a ? total_a : (src == e.slot_b ? total_b : *src);
                __hip_atomic_store(e.pub.dst + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            __hip_atomic_store(e.pub.seq_word, e.pub.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---- J*x for n > LSQ_LDS_X_MAX: x passes through LDS one column window at a time --------------------
// Block b = row block * ncw + window holds the rows' entries inside that window (rows without entries there have no
// lane).  The row block's workgroup walks the windows in ascending order; a lane CONTINUES the row's running sum from the
// output window in LDS (sum = yw[pos]; sum += products in column order; yw[pos] = sum), so every row is still one
// left-to-right sum over its entries -- the reference's order, bit for bit, as in k_sell_rows.
// A (row block, window) holds few entries per row (n = 50000, 10 per row: two), so its slices are short and a wave that
// took them one after the other would spend its time in memory round trips with 1-2 KB in flight.  Instead a wave requests
// the first two pairs of ALL its slices of the window (<= 4: 4096 rows = 64 slices over 16 waves) together with the window
// of x, before the barrier that hands the window over; their descriptors were requested during the previous window.  Only
// rows with more than four entries inside one window pay further round trips.
// 512 threads (8 waves, one workgroup per CU: 256 VGPRs per lane) so that the heads of a wave's 8 slices, the window of x and
// the next window's descriptors are all live in registers at once; with 1024 threads (128 VGPRs) the same code spilled.
constexpr int LSQ_WIDE_NT = 512;
// Width cap of a column window: 12544 doubles (98 KB) beside the 32 KB output window.  A little more than LSQ_LDS_X_MAX so
// that n <= 25088 needs TWO windows: measured at 10^6 x 25000 (nnz 10^7) 39.9 / 35.8 / 32.8 us with 5 / 4 / 3 windows.
constexpr int LSQ_SELL_WIDE_X_MAX = 12544;
constexpr int LSQ_SELL_WIDE_G = LSQ_SELL_ROWS_MAX / 64 / (LSQ_WIDE_NT / 64);   // slices per wave and (row block, window)

template <class Epi>
__global__ void __launch_bounds__(LSQ_WIDE_NT) k_sell_rows_wide(SellDev S, int wrows, int m, int ncw, int cwidth,
                                                                const double *__restrict__ x, int nx, Epi epi) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double sh[LSQ_WIDE_NT / 64];
    constexpr int NW = LSQ_WIDE_NT / 64, G = LSQ_SELL_WIDE_G;
    double *xl = smem;              // cwidth doubles (cwidth even)
    double *yw = smem + cwidth;     // LSQ_SELL_ROWS_MAX doubles
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nrb = S.nblocks / ncw;
    constexpr int XR = (LSQ_SELL_WIDE_X_MAX + LSQ_WIDE_NT - 1) / LSQ_WIDE_NT;
    constexpr int Q = LSQ_SELL_ROWS_MAX / LSQ_WIDE_NT;
    SellSliceRef A[G];
    double xr[XR];
    auto refs_at = [&](int w, int cw) {   // descriptors of this wave's slices of (row block w, window cw)
        const int sb = (w * ncw + cw) * S.spw;
#pragma unroll
        for (int g = 0; g < G; ++g) A[g] = sell_slice_ref(S, sb + wv + g * NW, sb + S.spw, lane);
    };
    auto fetch_x = [&](int cw) {
        const int c0 = cw * cwidth;
#pragma unroll
        for (int q = 0; q < XR; ++q) xr[q] = x[min(c0 + tid + q * LSQ_WIDE_NT, nx - 1)];
    };
    if ((int)blockIdx.x < nrb) refs_at(blockIdx.x, 0);
    const int dflag = epi.done ? *epi.done : 0;
    if constexpr (EpiHasBlockPrepare<Epi>::value) epi.block_prepare();
    if constexpr (EpiHasPrepare<Epi>::value) epi.prepare();
    if (dflag) return;   // launches queued behind a finished solve stop here
    double racc = 0.0;
    for (int w = blockIdx.x; w < nrb; w += gridDim.x) {
        const int base = w * wrows, rows = min(wrows, m - base);
        for (int cw = 0; cw < ncw; ++cw) {
            // the window of x and the head of every slice of this window: requested before anything is waited for
            // (measured and dropped: the NEXT window of x requested behind the LDS write, to travel during the sums -- its 48
            //  registers live across the sums made the kernel spill 75, 45 us instead of 33 at n = 25000)
            fetch_x(cw);
            SellSliceRef a[G];
            SellBatch<2> B[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                a[g] = A[g];
                const size_t oa = (size_t)a[g].sm.x + lane * 2;   // (an empty slice: a valid address, nothing selected)
                sell_batch_load<2, true>(B[g], S.val + oa, S.idx16 + oa, 0, max(a[g].sm.y >> 1, 1));
            }
            const bool more = cw + 1 < ncw, next_block = w + (int)gridDim.x < nrb;
            if (more) refs_at(w, cw + 1);
            else if (next_block) refs_at(w + gridDim.x, 0);
            __syncthreads();   // the previous window's gathers / the previous block's epilogue are done with xl, yw
#pragma unroll
            for (int q = 0; q < XR; ++q)
                if (tid + q * LSQ_WIDE_NT < cwidth) xl[tid + q * LSQ_WIDE_NT] = xr[q];
            if (cw == 0) {
#pragma unroll
                for (int q = 0; q < Q; ++q) yw[tid + q * LSQ_WIDE_NT] = 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int g = 0; g < G; ++g) {
                // (the column-windowed layout keeps EVEN slices -- build_sell's allow_odd = false: this kernel holds the heads of eight
                //  slices, a window of x and the next descriptors in 256 registers, and every form of the unpaired-entry path spilled)
                const int np = a[g].sm.y >> 1, len = (int)(a[g].inf >> LSQ_SELL_POS_BITS);
                const unsigned pos = a[g].inf & LSQ_SELL_POS_MASK;
                if (np == 0) continue;   // (wave-uniform)
                double sum = pos != LSQ_SELL_POS_MASK ? yw[pos] : 0.0, sq = 0.0;
                sell_batch_sum<2, true, false>(B[g], 0, np, len, xl, sum, sq);
                if (pos != LSQ_SELL_POS_MASK) yw[pos] = sum;
            }
            // rows with more than four entries inside the window: the rest of their slices, one slice after the other
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (a[g].sm.y <= 4) continue;   // (wave-uniform)
                const unsigned pos = a[g].inf & LSQ_SELL_POS_MASK;
                const size_t oa = (size_t)a[g].sm.x + lane * 2;
                double sum = pos != LSQ_SELL_POS_MASK ? yw[pos] : 0.0, sq = 0.0;
                sell_lane_sum_from<false, false>(S.val + oa, S.idx16 + oa, 2, a[g].sm.y, (int)(a[g].inf >> LSQ_SELL_POS_BITS), xl, sum, sq, lane);
                if (pos != LSQ_SELL_POS_MASK) yw[pos] = sum;
            }
        }
        double pre[Q];
        if constexpr (EpiHasPre<Epi>::value) {
#pragma unroll
            for (int q = 0; q < Q; ++q) pre[q] = epi.pre(base + min(tid + q * LSQ_WIDE_NT, rows - 1));
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = tid + q * LSQ_WIDE_NT;
            if (i < rows) {
                if constexpr (EpiHasPre<Epi>::value) epi.seg_pre(base + i, yw[i], pre[q], racc);
                else epi.seg(base + i, yw[i], racc);
            }
        }
    }
    for (int e = blockIdx.x; e < epi.extra_blocks; e += gridDim.x)
        if (tid < LSQ_NT) epi.extra(e, racc);
    finish_block_nt<LSQ_WIDE_NT>(epi, racc, sh);
}

// out = a .* b (the gather vector of a column-scaled wide handle: s .* x, formed once instead of once per row block)
template <int = 0>
__global__ void __launch_bounds__(LSQ_NT) k_sell_vmul(int n, const double *__restrict__ a, const double *__restrict__ b,
                                                      double *__restrict__ out) {
    for (int i = blockIdx.x * LSQ_NT + threadIdx.x; i < n; i += gridDim.x * LSQ_NT) out[i] = a[i] * b[i];
}

// ---- J'*y: per (gather window, column) partial sums; k_combine adds the windows ----------------
// block b = gw * ncb + cb; part layout [gw][n] (SQ: [gw][2n] = dots | squares)
// window of y -> LDS, all loads of a thread issued before the first use
__device__ __forceinline__ SellStageTail sell_cols_stage_y(int b, int ncb, int grows, int m, const double *__restrict__ y, double *yl,
                                                          int tid) {
    constexpr int YR = LSQ_SELL_GROWS_MAX / LSQ_BIG_NT;
    const int gw = b / ncb, gbase = gw * grows, rows = min(grows, m - gbase);
    SellStageTail t;
    t.v = 0.0;
    t.at = -1;
    if (sell_stage_dma_ok(y + gbase)) {        // (workgroup-uniform; window bases are multiples of 64 rows)
        // the zero fill past `rows` (the last window only) BEFORE the DMA is issued: plain LDS writes, nothing to wait for
        if (rows < grows) {
#pragma unroll
            for (int j = 0; j < YR; ++j) {
                const int i = tid + j * LSQ_BIG_NT;
                if (i >= rows && i < grows) yl[i] = 0.0;
            }
        }
        return sell_stage_dma<YR / 2>(y + gbase, yl, rows, tid);
    }
    double yr[YR];
#pragma unroll
    for (int j = 0; j < YR; ++j) yr[j] = y[gbase + min(tid + j * LSQ_BIG_NT, rows - 1)];
#pragma unroll
    for (int j = 0; j < YR; ++j)
        if (tid + j * LSQ_BIG_NT < grows) yl[tid + j * LSQ_BIG_NT] = (tid + j * LSQ_BIG_NT < rows) ? yr[j] : 0.0;
    sell_stage_wait();      // (nothing left that counts as pending: see sell_stage_dma)
    return t;
}
// the workgroup's blocks: a CONTIGUOUS run of block indices (blocks of one gather window are consecutive, so a workgroup that
// holds several blocks -- wide n: 1280 blocks at n = 50000 -- re-stages its 128 KB window of y only when the window changes,
// not once per block); the y window of the first one is already on its way to LDS (sell_cols_stage_y)
// XCD-aware placement (lsq_xcd_block): the blocks of one gather window (its column blocks) read the same 128 KB of y, so they
// should sit behind ONE L2 -- with runs dealt round-robin the four column blocks of a C4 gather window landed on four XCDs and
// every window of y was fetched four times (32 MB instead of 8 per launch).
__device__ __forceinline__ int sell_cols_wg() { return lsq_xcd_block((int)blockIdx.x, (int)gridDim.x); }
__device__ __forceinline__ int sell_cols_first(int nblocks) {
    const int per = (nblocks + (int)gridDim.x - 1) / (int)gridDim.x;
    return sell_cols_wg() * per;
}
template <bool SQ>
__device__ __forceinline__ void sell_cols_pass(const SellDev &S, int ncb, int ccols, int grows, int m, int n,
                                               const double *__restrict__ y, double *__restrict__ part, double *smem,
                                               SellStageTail ytail, int dflag, const SellSliceRef &ref0) {
    double *yl = smem;                          // LSQ_SELL_GROWS_MAX doubles
    double *ow = smem + LSQ_SELL_GROWS_MAX;     // LSQ_SELL_CCOLS_MAX doubles
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (S.nblocks + (int)gridDim.x - 1) / (int)gridDim.x;
    const int b0 = sell_cols_wg() * per, b1 = min(S.nblocks, b0 + per);
    for (int b = b0; b < b1; ++b) {
        const int gw = b / ncb, cb = b - gw * ncb;
        const int cbase = cb * ccols, cols = min(ccols, n - cbase);
        if (b != b0) {
            __syncthreads();   // the previous block's output pass is done with ow (and its gathers with yl)
            if (gw != (b - 1) / ncb) ytail = sell_cols_stage_y(b, ncb, grows, m, y, yl, tid);
        }
        const int s0 = b * S.spw, s1 = s0 + S.spw;
        double *dst = part + (size_t)gw * (SQ ? 2 : 1) * n + cbase;
        const bool stopped = sell_wave_slices<SQ>(S, s0, s1, wv, lane, yl, [&](unsigned pos, double sum, double sq) {   // (lane = one column)
            ow[pos] = sum;
            // (the squares -- the gradient + colsumabs2 pass of multiplied-out matrices, once per g! -- go straight to
            //  memory: a second LDS staging buffer would not fit next to the 128 KiB window)
            if constexpr (SQ) dst[n + pos] = sq;
        }, SellNoSliceHook(), [&]() {
            sell_stage_tail_write(ytail, yl);
            sell_stage_wait();      // (nothing of a DMA is outstanding at the barrier; the first batch is waited for with it)
        }, dflag, b == b0, ref0);
        if (stopped) return;        // (a launch queued behind a finished solve: behind the first barrier)
        ytail.at = -1;
        __syncthreads();
        for (int i = tid; i < cols; i += LSQ_BIG_NT) dst[i] = ow[i];
        sell_stage_wait();      // (nothing of this block counts as pending at the loop's head: see k_sell_rows)
    }
}

template <bool SQ>
__global__ void __launch_bounds__(LSQ_BIG_NT) k_sell_cols(SellDev S, int ncb, int ccols, int grows, int m, int n,
                                                          const double *__restrict__ y, double *__restrict__ part,
                                                          const int *done) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // the first window and the first slice's batch are requested together with the `done` flag of a finished solve (one latency,
    // not two in a row); the flag is acted on behind the first barrier, where no DMA is outstanding
    const int dflag = done ? *done : 0;
    const int bf = sell_cols_first(S.nblocks);
    // (the first slice's descriptor: requested ahead of the DMA, see sell_wave_slices)
    const SellSliceRef ref0 = sell_slice_ref(S, bf * S.spw + (int)(threadIdx.x >> 6), bf < S.nblocks ? (bf + 1) * S.spw : 0, threadIdx.x & 63);
    SellStageTail ytail;
    ytail.v = 0.0;
    ytail.at = -1;
    if (sell_cols_first(S.nblocks) < S.nblocks)
        ytail = sell_cols_stage_y(sell_cols_first(S.nblocks), ncb, grows, m, y, smem, threadIdx.x);
    if (bf >= S.nblocks) {      // (no block, nothing staged; otherwise the flag is acted on behind the first barrier)
        int d = dflag;
        asm volatile("" : "+v"(d));
        if (d) return;
    }
    sell_cols_pass<SQ>(S, ncb, ccols, grows, m, n, y, part, smem, ytail, dflag, ref0);
}
