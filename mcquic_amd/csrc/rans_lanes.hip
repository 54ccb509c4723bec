// Lane-interleaved rANS streams on the device, for gfx950: the coder of rans_dev.hip with a WAVE, not a lane, as the unit of work.
//
// rans_dev.hip keeps the reference's format, one 64-bit state per stream, so a stream is one lane's dependent chain.  The layout here
// (include/mcquic_hip.h, "lane-interleaved streams"; host side rans.cpp) carries W in {1, 2, ..., 64} states over ONE sequence of 32-bit
// words: within group g, round r holds positions r W + l, lane l owns state l, and the chain a stream waits for is hw / W steps per group.
// Per-state arithmetic is rans_dev.hip's, spelled the same way -- uint64_t `/` and `%`, L = 2^31, 16-bit probabilities.
//   words as read   prefix 'M' 'Q' 'L' W | 2 W state words, lane 0 first | per round the words of the lanes that renormalise, lowest first
// One wave per stream, all levels and images in ONE launch on rans_dev.hip's grid (level, image); stream s = image * row_levels + level0 +
// level.  Plain stores, no atomics, nothing allocated: both entry points capture into a graph.
//
//   rans_lanes_encode_kernel   groups m - 1 .. 0, rounds last to first.  Per group the rounds are taken in chunks of MCQ_RANS_DEV_CHUNK / W:
//                        all 64 lanes gather (start, freq) of the chunk's positions -- a coalesced read of the int64 codes, two table reads
//                        each -- into LDS as one word; a code outside [0, k) or a width of 0 is found HERE, before anything is indexed
//                        with it, sets the stream's status and makes its size 0 (as rans_encode_kernel).  Then round by round: every
//                        active lane tests x >= freq << 47, ONE ballot collects the lanes that emit, and a lane's slot among the round's
//                        words is the popcount of the ballot below it (lanes of a round read forwards lowest first; the words fill the LDS
//                        array from its END).  When fewer than 64 slots are left the array moves to the stream's scratch slot, which fills
//                        from its end too.  Last come the 2 W state words and the prefix.  A step emits at most one word per lane:
//                        4 (1 + 2 W + m hw) bytes always suffice and the launcher refuses a smaller slot.  The blob is packed by
//                        rans_dev.hip's rans_scan_kernel / rans_copy_kernel through mcq_rans_pack_dev, unchanged.
//   rans_lanes_decode_kernel   the group's table in LDS (as rans_decode_kernel), stream words staged in LDS by the chunk.  Every lane has its
//                        OWN cum here, so the wave-cooperative ballot search of rans_decode_kernel -- 64 lanes probing for one cum -- does
//                        not apply: each lane bisects entries 1 .. k - 1 in LDS by itself, ceil(log2 k) <= 13 dependent ds_read_b32.  The
//                        first probe is one address for the whole wave (a broadcast); later probes scatter over the 32 banks as the
//                        states dictate, so a probe costs what its worst bank holds -- data-dependent, not a layout to pad away.  The search
//                        cannot leave the table whatever it holds, and a bin that does not contain cum sets the status.  Word fetch: one
//                        ballot of the lanes with x < L, lane l takes word wnext + popcount(ballot below l); wnext + count is tested against
//                        the stream's word count BEFORE the read, and the staged chunk is refilled (guarded the same way) when the round's
//                        words reach past it.  Symbols are stored as int64 straight to the output: a round is W consecutive elements.
//                        Untrusted input: the extent is checked as in rans_decode_kernel, then the prefix, W and 4 (1 + 2 W) bytes; every
//                        refusal sets this stream's status alone and zeroes its codes.  W comes from the prefix and from nothing else.
#include "mcq_common.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int LANES_CH = MCQ_RANS_DEV_CHUNK;        // symbols / words per LDS chunk
constexpr int LANES_T = 64;                         // one wave per stream
constexpr int LANES_KMAX = MCQ_CDF_MAX_K;
constexpr unsigned long long LANES_L = 1ull << 31;

struct LanesEncK {
    const long long* codes[MCQ_VQ_MAX_LEVELS];      // level l: [n, m_l, h_l, w_l]
    const uint32_t* cdf[MCQ_VQ_MAX_LEVELS];         // level l: [m_l, k_l + 1]
    int32_t m[MCQ_VQ_MAX_LEVELS];
    int32_t k[MCQ_VQ_MAX_LEVELS];
    int32_t hw[MCQ_VQ_MAX_LEVELS];
    int32_t lanes[MCQ_VQ_MAX_LEVELS];               // W_l, resolved on the host
    int32_t level0, row_levels;
    uint32_t* scratch;                              // [streams, cap_words]
    long long cap_words;
    long long* sizes;                               // [streams] bytes
    int32_t* status;                                // [streams]
};

__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

__global__ __launch_bounds__(LANES_T) void rans_lanes_encode_kernel(LanesEncK q) {
    __shared__ uint32_t pair[LANES_CH];             // start << 16 | freq, both as uint16; position base + j of the group
    __shared__ uint32_t word[LANES_CH];             // words not yet in the scratch slot, filled from the end
    const int lv = (int)blockIdx.x, img = (int)blockIdx.y, lane = (int)threadIdx.x;
    const int m = q.m[lv], k = q.k[lv], hw = q.hw[lv], W = q.lanes[lv];
    const size_t s = (size_t)img * q.row_levels + q.level0 + lv;
    const long long* code = q.codes[lv] + (size_t)img * m * hw;
    uint32_t* slot_end = q.scratch + (s + 1) * (size_t)q.cap_words;
    const int rounds = (hw + W - 1) / W;
    const int per = LANES_CH / W;                   // rounds per gathered chunk
    unsigned long long x = LANES_L;                 // lane l < W: state l
    long long total = 0;                            // words in the scratch slot so far
    int wp = LANES_CH;                              // word[wp ..] are staged

    for (int g = m; g-- > 0;) {
        const uint32_t* t = q.cdf[lv] + (size_t)g * (k + 1);
        const long long* cg = code + (size_t)g * hw;
        for (int r1 = rounds; r1 > 0;) {
            const int r0 = ((r1 - 1) / per) * per;
            const int base = r0 * W;
            const int len = (r1 * W < hw ? r1 * W : hw) - base;      // (<= per W <= LANES_CH)
            long long c[LANES_CH / LANES_T];
#pragma unroll
            for (int i = 0; i < LANES_CH / LANES_T; ++i) {
                const int j = lane + i * LANES_T;
                c[i] = j < len ? cg[base + j] : 0;
            }
            int bad = 0;
#pragma unroll
            for (int i = 0; i < LANES_CH / LANES_T; ++i) {
                const int j = lane + i * LANES_T;
                if (j < len) {
                    uint32_t p = 0;
                    if (c[i] >= 0 && c[i] < k) {    // tested before the table is indexed with it
                        const uint32_t start = t[c[i]], next = t[c[i] + 1];
                        p = (start & 0xffffu) << 16 | ((next - start) & 0xffffu);
                    }
                    bad |= (p & 0xffffu) == 0u;
                    pair[j] = p;
                }
            }
            if (__syncthreads_or(bad)) {            // (uniform) also publishes pair[]
                if (lane == 0) { q.sizes[s] = 0; q.status[s] = MCQ_RANS_BAD_SYMBOL; }
                return;
            }
            for (int r = r1; r-- > r0;) {
                if (wp < LANES_T) {                 // (uniform) a round may need 64 slots: move what is staged to the scratch slot
                    __syncthreads();
                    const int nw = LANES_CH - wp;
                    uint32_t* dst = slot_end - total - nw;      // (total + nw <= symbols so far <= cap_words - 2 W - 1)
                    for (int j = lane; j < nw; j += LANES_T) dst[j] = word[wp + j];
                    total += nw;
                    wp = LANES_CH;
                    __syncthreads();
                }
                const bool active = lane < W && r * W + lane < hw;
                const uint32_t p = active ? pair[(r - r0) * W + lane] : 1u;
                const uint32_t freq = p & 0xffffu, start = p >> 16;
                const bool emit = active && x >= ((unsigned long long)freq << 47);
                const unsigned long long mask = __ballot(emit);
                const int cnt = __popcll(mask);
                if (emit) { word[wp - cnt + lanes_below(mask, lane)] = (uint32_t)x; x >>= 32; }       // (cnt <= 64 <= wp)
                wp -= cnt;
                if (active) x = ((x / freq) << 16) + (x % freq) + start;
            }
            __syncthreads();                        // pair[] is rewritten by the next chunk
            r1 = r0;
        }
    }
    __syncthreads();
    const int nw = LANES_CH - wp;
    uint32_t* dst = slot_end - total - nw;
    for (int j = lane; j < nw; j += LANES_T) dst[j] = word[wp + j];
    total += nw;
    uint32_t* head = slot_end - total - 2 * W - 1;  // (total <= m hw: inside the slot, checked on the host)
    if (lane < W) {
        head[1 + 2 * lane] = (uint32_t)x;
        head[2 + 2 * lane] = (uint32_t)(x >> 32);
    }
    if (lane == 0) {
        head[0] = (uint32_t)MCQ_RANS_LANES_MAGIC | (uint32_t)W << 24;
        q.sizes[s] = 4 * (total + 2 * W + 1);
        q.status[s] = MCQ_RANS_OK;
    }
}

struct LanesDecK {
    long long* codes[MCQ_VQ_MAX_LEVELS];            // level l: [n, m_l, h_l, w_l]
    const uint32_t* cdf[MCQ_VQ_MAX_LEVELS];         // level l: [m_l, k_l + 1]
    int32_t m[MCQ_VQ_MAX_LEVELS];
    int32_t k[MCQ_VQ_MAX_LEVELS];
    int32_t hw[MCQ_VQ_MAX_LEVELS];
    int32_t level0, row_levels;
    const uint8_t* blob;
    long long blob_bytes;
    const long long* offsets;                       // [streams + 1]
    int32_t* status;                                // [streams]
};

// little-endian word j of a stream that starts at byte `in` (any alignment); the caller has tested j against the stream's word count
__device__ __forceinline__ uint32_t lanes_word(const uint8_t* in, long long j) {
    const uint8_t* b = in + 4 * j;
    return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

__global__ __launch_bounds__(LANES_T) void rans_lanes_decode_kernel(LanesDecK q) {
    __shared__ uint32_t table[LANES_KMAX + 1];      // the group's k + 1 entries
    __shared__ uint32_t word[LANES_CH];             // stream words [wbase, wbase + LANES_CH)
    const int lv = (int)blockIdx.x, img = (int)blockIdx.y, lane = (int)threadIdx.x;
    const int m = q.m[lv], k = q.k[lv], hw = q.hw[lv];
    const int count = m * hw;
    const size_t s = (size_t)img * q.row_levels + q.level0 + lv;
    long long* out = q.codes[lv] + (size_t)img * count;

    // the stream's extent, checked before anything is read through it
    const long long off0 = q.offsets[s], off1 = q.offsets[s + 1];
    const long long size = off1 - off0;
    int status = MCQ_RANS_OK;
    if (off0 < 0 || off1 < off0 || off1 > q.blob_bytes || (size & 3) || size < 4) status = MCQ_RANS_BAD_STREAM;
    const long long nwords = status ? 0 : size / 4;         // every word index below is tested against this
    const uint8_t* in = q.blob + (status ? 0 : off0);       // (a stream may start at any byte)

    for (int j = lane; j < LANES_CH; j += LANES_T) word[j] = j < nwords ? lanes_word(in, j) : 0u;
    __syncthreads();
    int W = 1;
    if (!status) {
        const uint32_t prefix = word[0];
        const int w = (int)(prefix >> 24);
        if ((prefix & 0xffffffu) != (uint32_t)MCQ_RANS_LANES_MAGIC || w < 1 || w > MCQ_RANS_LANES_MAX || (w & (w - 1)) || nwords < 1 + 2 * w)
            status = MCQ_RANS_BAD_STREAM;
        else
            W = w;
    }
    unsigned long long x = 0;
    if (!status && lane < W) x = (unsigned long long)word[1 + 2 * lane] | ((unsigned long long)word[2 + 2 * lane] << 32);      // (2 W + 1 <= 129 <= LANES_CH)
    long long wbase = 0, wnext = 1 + 2 * W;         // word[] holds stream words from wbase on; wnext = the next one to take
    const int rounds = (hw + W - 1) / W;

    for (int g = 0; g < m && !status; ++g) {        // (everything the loops branch on is the same in every lane)
        __syncthreads();
        const uint32_t* t = q.cdf[lv] + (size_t)g * (k + 1);
        for (int j = lane; j <= k; j += LANES_T) table[j] = t[j];
        __syncthreads();
        long long* og = out + (size_t)g * hw;
        for (int r = 0; r < rounds; ++r) {
            const int p = r * W + lane;
            const bool active = lane < W && p < hw;
            int bin = 0;
            bool wrong = false;
            if (active) {
                const uint32_t cum = (uint32_t)(x & 0xffffu);
                int lo = 1, hi = k;                 // the first of entries 1 .. k - 1 strictly above cum, less one: stays within [0, k)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (table[mid] > cum) hi = mid; else lo = mid + 1;
                }
                bin = lo - 1;
                const uint32_t start = table[bin], next = table[bin + 1];
                wrong = !(start <= cum && cum < next);          // not this bin's (the bisection has seen both entries unless they are the table's ends)
                x = (unsigned long long)(next - start) * (x >> 16) + cum - start;
            }
            if (__ballot(wrong)) { status = MCQ_RANS_BAD_STREAM; break; }
            const bool need = active && x < LANES_L;
            const unsigned long long mask = __ballot(need);
            const int cnt = __popcll(mask);
            if (cnt) {
                if (wnext + cnt > nwords) { status = MCQ_RANS_BAD_STREAM; break; }      // out of words
                if (wnext + cnt > wbase + LANES_CH) {                                   // the round's words reach past the staged chunk
                    __syncthreads();
                    wbase = wnext;
                    for (int j = lane; j < LANES_CH; j += LANES_T) word[j] = wbase + j < nwords ? lanes_word(in, wbase + j) : 0u;
                    __syncthreads();
                }
                if (need) x = (x << 32) | word[(int)(wnext - wbase) + lanes_below(mask, lane)];       // (< cnt <= 64 <= LANES_CH past wnext - wbase)
                wnext += cnt;
            }
            if (active) og[p] = (long long)bin;
        }
    }
    if (status)
        for (int j = lane; j < count; j += LANES_T) out[j] = 0;
    if (lane == 0) q.status[s] = status;
}

static_assert(LANES_CH % LANES_T == 0 && LANES_CH >= 2 * MCQ_RANS_LANES_MAX + 1 + LANES_T, "the head and a round's words fit one staged chunk");
static_assert(MCQ_RANS_LANES_MAX == LANES_T, "one state per lane of a wave");

// W for a level: the width asked for, or the auto rule (mcq_rans_lanes_auto, rans.cpp); 0 = refused
int lanes_width(int32_t lanes, long long symbols) {
    if (lanes == 0) return mcq_rans_lanes_auto(symbols);
    return lanes >= 1 && lanes <= MCQ_RANS_LANES_MAX && (lanes & (lanes - 1)) == 0 ? lanes : 0;
}

}  // namespace

extern "C" int mcq_rans_lanes_encode_dev(const int64_t* const* codes, const uint32_t* const* cdf, const int32_t* m, const int32_t* k,
                                         const int32_t* hw, const int32_t* lanes, int32_t levels, int32_t n, int32_t level0, int32_t row_levels,
                                         uint8_t* scratch, int64_t cap_bytes, int64_t* sizes, int32_t* status, void* stream) {
    if (!codes || !cdf || !m || !k || !hw || !lanes || !scratch || !sizes || !status || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return MCQ_EINVAL;
    if (n <= 0 || level0 < 0 || row_levels < level0 + levels || cap_bytes < 12 || (cap_bytes & 3) || ((uintptr_t)scratch & 3)) return MCQ_EINVAL;
    if (n > 65535) return MCQ_ETOOLARGE;            // (grid y)
    LanesEncK q;
    for (int l = 0; l < levels; ++l) {
        if (!codes[l] || !cdf[l] || m[l] <= 0 || k[l] <= 0 || hw[l] <= 0 || k[l] > LANES_KMAX) return MCQ_EINVAL;
        const long long count = (long long)m[l] * hw[l];
        if (count > MCQ_RANS_DEV_MAX_SYMBOLS) return MCQ_ETOOLARGE;
        const int W = lanes_width(lanes[l], count);
        if (W == 0) return MCQ_EINVAL;
        if (4 * (count + 2 * W + 1) > cap_bytes) return MCQ_EINVAL;        // the slot could not hold the worst case
        q.codes[l] = reinterpret_cast<const long long*>(codes[l]); q.cdf[l] = cdf[l];
        q.m[l] = m[l]; q.k[l] = k[l]; q.hw[l] = hw[l]; q.lanes[l] = W;
    }
    q.level0 = level0; q.row_levels = row_levels; q.scratch = reinterpret_cast<uint32_t*>(scratch); q.cap_words = cap_bytes / 4;
    q.sizes = reinterpret_cast<long long*>(sizes); q.status = status;
    hipLaunchKernelGGL(rans_lanes_encode_kernel, dim3((unsigned)levels, (unsigned)n), dim3(LANES_T), 0, (hipStream_t)stream, q);
    return mcq_check_launch();
}

extern "C" int mcq_rans_lanes_decode_dev(const uint8_t* blob, int64_t blob_bytes, const int64_t* offsets, const uint32_t* const* cdf,
                                         const int32_t* m, const int32_t* k, const int32_t* hw, int32_t levels, int32_t n, int32_t level0,
                                         int32_t row_levels, int64_t* const* codes, int32_t* status, void* stream) {
    if (!blob || !offsets || !cdf || !m || !k || !hw || !codes || !status || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return MCQ_EINVAL;
    if (n <= 0 || level0 < 0 || row_levels < level0 + levels || blob_bytes < 0) return MCQ_EINVAL;
    if (n > 65535) return MCQ_ETOOLARGE;            // (grid y)
    LanesDecK q;
    for (int l = 0; l < levels; ++l) {
        if (!codes[l] || !cdf[l] || m[l] <= 0 || k[l] <= 0 || hw[l] <= 0 || k[l] > LANES_KMAX) return MCQ_EINVAL;      // (the table is held in LDS)
        if ((long long)m[l] * hw[l] > MCQ_RANS_DEV_MAX_SYMBOLS) return MCQ_ETOOLARGE;
        q.codes[l] = reinterpret_cast<long long*>(codes[l]); q.cdf[l] = cdf[l];
        q.m[l] = m[l]; q.k[l] = k[l]; q.hw[l] = hw[l];
    }
    q.level0 = level0; q.row_levels = row_levels; q.blob = blob; q.blob_bytes = blob_bytes;
    q.offsets = reinterpret_cast<const long long*>(offsets); q.status = status;
    hipLaunchKernelGGL(rans_lanes_decode_kernel, dim3((unsigned)levels, (unsigned)n), dim3(LANES_T), 0, (hipStream_t)stream, q);
    return mcq_check_launch();
}
