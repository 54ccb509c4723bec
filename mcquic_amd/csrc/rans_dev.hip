// The entropy coder itself on the device, for gfx950: the rANS byte streams of the `.mcq` payload made and read where the codes live --
// no host loop, no host read, plain stores, no atomics, nothing allocated: every entry point captures into a graph.
//
// The format is rans.cpp's (CompressAI's cpp_exts over ryg_rans' rans64.h), bit for bit: one 64-bit state per stream, L = 2^31, 16-bit
// probabilities, symbols encoded in REVERSE, 32-bit words emitted BACKWARDS (so the decoder reads them forwards), the final state flushed
// as two words in front.  All arithmetic is integer and spelled as rans.cpp spells it -- uint64_t `/` and `%`, no reciprocal:
//   encode   if (x >= freq << 47) { emit (uint32)x; x >>= 32; }   x = ((x / freq) << 16) + (x % freq) + start        ((L >> 16) << 32 = 2^47)
//   decode   cum = x & 0xffff; s = the bin with cdf[s] <= cum < cdf[s + 1];
//            x = freq (x >> 16) + cum - start;   if (x < L) x = (x << 32) | next word
// A stream is sequential; streams are independent per (image, level): one workgroup per stream, all levels and images in ONE launch
// (the grid of vq_code_bits_kernel).  Stream s = image * row_levels + level0 + level: image-major, the order `binaries[n][level]` has.
//
//   rans_encode_kernel   256 lanes per stream.  The symbols code[i].flatten() ([m, h, w] order, the group index selecting the table) are
//                        taken in chunks of MCQ_RANS_DEV_CHUNK, last chunk first.  Per chunk ALL lanes gather (start, freq) -- a coalesced
//                        read of the int64 codes and two table reads each -- into LDS as one word, both halves truncated to 16 bits as
//                        rans.cpp's `Sym` holds them; a code outside [0, k) or a width of 0 (rans.cpp:119 and :139, MCQ_EINVAL) is
//                        found HERE, before anything is indexed with it, sets the stream's status and makes its size 0.  Then lane 0
//                        walks the recurrence over the chunk, last symbol first, and leaves the words it emits in LDS; all lanes move
//                        them to the stream's slot of the scratch buffer [streams, cap], which fills from its END towards its start.
//                        cap: rans64.h keeps L <= x < L << 32 = 2^63 between steps, so after one shift x < 2^31 < 2^47 <= freq << 47:
//                        a step emits at most ONE word, the flush two, and 4 (symbols + 2) bytes always suffice; the launcher refuses
//                        a smaller slot.  (The host side allocates 4 symbols + 64, rans.cpp's own margin.)
//   rans_scan_kernel     one workgroup: offsets[0 .. streams] = the exclusive scan of the sizes (every size a multiple of 4).
//   rans_copy_kernel     one workgroup per stream: its bytes from the end of its scratch slot to blob + offsets[s].  `offsets` and `blob`
//                        are what leaves the device: the coded bytes, not four per symbol.
//   rans_decode_kernel   ONE wave per stream; every lane carries the same state.  A stream visits its groups one after another, so a
//                        group's table (k + 1 <= 8193 entries) is staged in LDS once per group; stream words are staged in LDS by the
//                        chunk and the decoded symbols collected there and stored as int64, coalesced, straight into the level's
//                        [n, m, h, w] output -- no int32 staging, no widening pass.  The search for the bin is wave-cooperative: lane l
//                        probes entry 1 + l B (B = ceil((k - 1) / 64) <= 128), a ballot counts the probes <= cum, then the B entries of
//                        that block are probed 64 at a time and counted by ballot again: 2 to 3 LDS reads deep where one lane bisecting
//                        reads 13 times, each dependent on the one before.  Chosen by reading the code; the two have NOT been measured
//                        against each other.  Whatever the table holds the count stays within [0, k): the search cannot leave the table,
//                        and a bin that does not contain cum (a table that is not increasing) sets the status.
//                        The stream is untrusted input (it comes out of a `.mcq` file): a size below 8 bytes or not a multiple of 4,
//                        offsets that decrease or reach beyond blob_bytes, and running out of words each set the stream's
//                        status and stop that stream only.  Every read of a stream word is guarded by the stream's own word count, which
//                        is formed from offsets already checked against blob_bytes -- no malformed input reaches a load.  A stream with a
//                        status leaves its outputs zeroed.
//
// Not on the device: the 4-bit bypass digits (a value at or beyond a table's sentinel slot).  With the product's cdfSizes = k + 2 over
// k + 1 entries the sentinel is k, which no code index in [0, k) reaches: on the host the branch is kept for format completeness, here
// such a code is the status word.  Streams written by either side read back on the other.
#include "mcq_common.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int RANS_CH = MCQ_RANS_DEV_CHUNK;         // symbols / words per LDS chunk
constexpr int RANS_ENC_T = 256;                     // lanes of an encoder workgroup
constexpr int RANS_DEC_T = 64;                      // one wave decodes a stream
constexpr int RANS_SCAN_T = 1024;
constexpr int RANS_KMAX = MCQ_CDF_MAX_K;            // the longest table the decoder's LDS array holds
constexpr unsigned long long RANS_L = 1ull << 31;

struct RansEncK {
    const long long* codes[MCQ_VQ_MAX_LEVELS];      // level l: [n, m_l, h_l, w_l]
    const uint32_t* cdf[MCQ_VQ_MAX_LEVELS];         // level l: [m_l, k_l + 1]
    int32_t m[MCQ_VQ_MAX_LEVELS];
    int32_t k[MCQ_VQ_MAX_LEVELS];
    int32_t hw[MCQ_VQ_MAX_LEVELS];
    int32_t level0, row_levels;
    uint32_t* scratch;                              // [streams, cap_words]
    long long cap_words;
    long long* sizes;                               // [streams] bytes
    int32_t* status;                                // [streams]
};

__global__ __launch_bounds__(RANS_ENC_T) void rans_encode_kernel(RansEncK q) {
    __shared__ uint32_t pair[RANS_CH];              // start << 16 | freq, both as uint16
    __shared__ uint32_t word[RANS_CH];              // the words of this chunk, filled from the end
    __shared__ int wfirst;
    const int lv = (int)blockIdx.x, img = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int m = q.m[lv], k = q.k[lv], hw = q.hw[lv];
    const int count = m * hw;                       // (<= MCQ_RANS_DEV_MAX_SYMBOLS: checked on the host)
    const size_t s = (size_t)img * q.row_levels + q.level0 + lv;
    const long long* code = q.codes[lv] + (size_t)img * count;
    const uint32_t* cdf = q.cdf[lv];
    uint32_t* slot_end = q.scratch + (s + 1) * (size_t)q.cap_words;
    unsigned long long x = RANS_L;                  // (lane 0's is the stream's)
    long long total = 0;                            // words stored so far

    for (int lo = ((count - 1) / RANS_CH) * RANS_CH; lo >= 0; lo -= RANS_CH) {
        const int len = count - lo < RANS_CH ? count - lo : RANS_CH;
        int bad = 0;
        for (int j = tid; j < len; j += RANS_ENC_T) {
            const long long c = code[lo + j];
            uint32_t p = 0;
            if (c >= 0 && c < k) {                  // tested before the table is indexed with it
                const uint32_t* t = cdf + (size_t)((lo + j) / hw) * (k + 1);
                const uint32_t start = t[c], next = t[c + 1];
                p = (start & 0xffffu) << 16 | ((next - start) & 0xffffu);
            }
            bad |= (p & 0xffffu) == 0u;
            pair[j] = p;
        }
        if (__syncthreads_or(bad)) {                // (uniform) also publishes pair[]
            if (tid == 0) { q.sizes[s] = 0; q.status[s] = MCQ_RANS_BAD_SYMBOL; }
            return;
        }
        if (tid == 0) {
            int wp = RANS_CH;
            for (int j = len; j-- > 0;) {
                const uint32_t p = pair[j];
                const uint32_t freq = p & 0xffffu, start = p >> 16;
                if (x >= ((unsigned long long)freq << 47)) { word[--wp] = (uint32_t)x; x >>= 32; }      // (at most one per symbol: wp >= 0)
                x = ((x / freq) << 16) + (x % freq) + start;
            }
            wfirst = wp;
        }
        __syncthreads();
        const int wp = wfirst, nw = RANS_CH - wp;
        uint32_t* dst = slot_end - total - nw;      // (total + nw <= symbols so far <= cap_words - 2)
        for (int j = tid; j < nw; j += RANS_ENC_T) dst[j] = word[wp + j];
        total += nw;
        __syncthreads();                            // word[] and pair[] are rewritten by the next chunk
    }
    if (tid == 0) {
        uint32_t* dst = slot_end - total - 2;
        dst[0] = (uint32_t)x;
        dst[1] = (uint32_t)(x >> 32);
        q.sizes[s] = 4 * (total + 2);
        q.status[s] = MCQ_RANS_OK;
    }
}

// exclusive scan of one value per lane over the workgroup, lane order; *total = the sum
__device__ __forceinline__ long long rans_block_scan(long long v, long long* sm, long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long sum = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long u = __shfl_up(sum, off);
        if (lane >= off) sum += u;
    }
    if (lane == 63) sm[wave] = sum;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RANS_SCAN_T / 64; ++w) {
        const long long t = sm[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();
    *total = all;
    return sum - v + before;
}

__global__ __launch_bounds__(RANS_SCAN_T) void rans_scan_kernel(const long long* sizes, long long streams, long long* offsets) {
    __shared__ long long sm[RANS_SCAN_T / 64];
    long long carry = 0;
    for (long long s0 = 0; s0 < streams; s0 += RANS_SCAN_T) {
        const long long s = s0 + threadIdx.x;
        const long long v = s < streams ? sizes[s] : 0;
        long long all;
        const long long at = rans_block_scan(v, sm, &all);
        if (s < streams) offsets[s] = carry + at;
        carry += all;
    }
    if (threadIdx.x == 0) offsets[streams] = carry;
}

__global__ __launch_bounds__(256) void rans_copy_kernel(const uint32_t* scratch, long long cap_words, const long long* sizes,
                                                        const long long* offsets, uint32_t* blob, long long blob_bytes) {
    const size_t s = blockIdx.x;
    const long long size = sizes[s], off = offsets[s];
    if (size <= 0 || size > 4 * cap_words || off < 0 || off + size > blob_bytes) return;      // (not with a blob of the worst-case size)
    const uint32_t* src = scratch + (s + 1) * (size_t)cap_words - size / 4;
    uint32_t* dst = blob + off / 4;
    for (long long j = threadIdx.x; j < size / 4; j += 256) dst[j] = src[j];
}

struct RansDecK {
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
__device__ __forceinline__ uint32_t rans_word(const uint8_t* in, long long j) {
    const uint8_t* b = in + 4 * j;
    return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

__global__ __launch_bounds__(RANS_DEC_T) void rans_decode_kernel(RansDecK q) {
    __shared__ uint32_t table[RANS_KMAX + 1];       // the group's k + 1 entries
    __shared__ uint32_t word[RANS_CH];              // stream words [wbase, wbase + RANS_CH)
    __shared__ uint16_t sym[RANS_CH];               // decoded symbols [i - i % RANS_CH, i]
    const int lv = (int)blockIdx.x, img = (int)blockIdx.y, lane = (int)threadIdx.x;
    const int m = q.m[lv], k = q.k[lv], hw = q.hw[lv];
    const int count = m * hw;
    const size_t s = (size_t)img * q.row_levels + q.level0 + lv;
    long long* out = q.codes[lv] + (size_t)img * count;
    const uint32_t* cdf = q.cdf[lv];

    // the stream's extent, checked before anything is read through it
    const long long off0 = q.offsets[s], off1 = q.offsets[s + 1];
    const long long size = off1 - off0;
    int status = MCQ_RANS_OK;
    if (off0 < 0 || off1 < off0 || off1 > q.blob_bytes || (size & 3) || size < 8) status = MCQ_RANS_BAD_STREAM;
    const long long nwords = status ? 0 : size / 4;         // every word index below is tested against this
    const uint8_t* in = q.blob + (status ? 0 : off0);       // (a stream may start at any byte: a neighbour's length need not be a multiple of 4)

    unsigned long long x = 0;
    long long wbase = 0, wnext = 2;                 // word[] holds stream words from wbase on; wnext = the next one to take
    if (!status) {
        for (int j = lane; j < RANS_CH; j += RANS_DEC_T) word[j] = j < nwords ? rans_word(in, j) : 0u;
        __syncthreads();
        x = (unsigned long long)word[0] | ((unsigned long long)word[1] << 32);
    }
    const int span = k - 1;                         // the search runs over entries 1 .. k - 1
    const int B = (span + 63) / 64;                 // (<= 128)
    int group_end = 0, g = 0;
    for (int i = 0; i < count && !status; ++i) {    // (everything the loop branches on is the same in every lane)
        if (i == group_end) {                       // the next group's table
            __syncthreads();
            const uint32_t* t = cdf + (size_t)g * (k + 1);
            for (int j = lane; j <= k; j += RANS_DEC_T) table[j] = t[j];
            __syncthreads();
            ++g;
            group_end += hw;
        }
        const uint32_t cum = (uint32_t)(x & 0xffffu);
        // first entry strictly above cum, less one = how many of the entries 1 .. k - 1 are <= cum
        int bin = 0;
        {
            const int at = 1 + lane * B;
            const int c = __popcll(__ballot(at <= span && table[at] <= cum));
            bin = c;
            if (B > 1 && c > 0) {
                const int base = 1 + (c - 1) * B;
                int inside = 0;
                for (int r = 0; r < B; r += 64) {
                    const int e = base + r + lane;
                    inside += __popcll(__ballot(r + lane < B && e <= span && table[e] <= cum));
                }
                bin = (c - 1) * B + inside;
            }
            bin = bin < k ? bin : k - 1;            // (never taken with an increasing table; keeps bin + 1 <= k for any other)
        }
        const uint32_t start = table[bin], freq = table[bin + 1] - start;
        if (cum - start >= freq) { status = MCQ_RANS_BAD_STREAM; break; }      // not this bin's: the table is not increasing
        x = (unsigned long long)freq * (x >> 16) + cum - start;
        if (x < RANS_L) {
            if (wnext >= nwords) { status = MCQ_RANS_BAD_STREAM; break; }      // out of words
            if (wnext >= wbase + RANS_CH) {         // the next chunk of the stream
                __syncthreads();
                wbase = wnext;
                for (int j = lane; j < RANS_CH; j += RANS_DEC_T) word[j] = wbase + j < nwords ? rans_word(in, wbase + j) : 0u;
                __syncthreads();
            }
            x = (x << 32) | word[wnext - wbase];
            ++wnext;
        }
        const int slot = i & (RANS_CH - 1);
        if (lane == 0) sym[slot] = (uint16_t)bin;
        if (slot == RANS_CH - 1 || i == count - 1) {
            __syncthreads();
            const int first = i - slot;
            for (int j = lane; j <= slot; j += RANS_DEC_T) out[first + j] = (long long)sym[j];
            __syncthreads();
        }
    }
    if (status)
        for (int j = lane; j < count; j += RANS_DEC_T) out[j] = 0;
    if (lane == 0) q.status[s] = status;
}

static_assert((RANS_CH & (RANS_CH - 1)) == 0, "the chunk index is a mask");

}  // namespace

extern "C" int mcq_rans_encode_dev(const int64_t* const* codes, const uint32_t* const* cdf, const int32_t* m, const int32_t* k, const int32_t* hw,
                                   int32_t levels, int32_t n, int32_t level0, int32_t row_levels, uint8_t* scratch, int64_t cap_bytes,
                                   int64_t* sizes, int32_t* status, void* stream) {
    if (!codes || !cdf || !m || !k || !hw || !scratch || !sizes || !status || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return MCQ_EINVAL;
    if (n <= 0 || level0 < 0 || row_levels < level0 + levels || cap_bytes < 8 || (cap_bytes & 3) || ((uintptr_t)scratch & 3)) return MCQ_EINVAL;
    if (n > 65535) return MCQ_ETOOLARGE;            // (grid y)
    RansEncK q;
    for (int l = 0; l < levels; ++l) {
        if (!codes[l] || !cdf[l] || m[l] <= 0 || k[l] <= 0 || hw[l] <= 0 || k[l] > RANS_KMAX) return MCQ_EINVAL;
        const long long count = (long long)m[l] * hw[l];
        if (count > MCQ_RANS_DEV_MAX_SYMBOLS) return MCQ_ETOOLARGE;
        if (4 * (count + 2) > cap_bytes) return MCQ_EINVAL;        // the slot could not hold the worst case
        q.codes[l] = reinterpret_cast<const long long*>(codes[l]); q.cdf[l] = cdf[l];
        q.m[l] = m[l]; q.k[l] = k[l]; q.hw[l] = hw[l];
    }
    q.level0 = level0; q.row_levels = row_levels; q.scratch = reinterpret_cast<uint32_t*>(scratch); q.cap_words = cap_bytes / 4;
    q.sizes = reinterpret_cast<long long*>(sizes); q.status = status;
    hipLaunchKernelGGL(rans_encode_kernel, dim3((unsigned)levels, (unsigned)n), dim3(RANS_ENC_T), 0, (hipStream_t)stream, q);
    return mcq_check_launch();
}

extern "C" int mcq_rans_pack_dev(const uint8_t* scratch, int64_t cap_bytes, const int64_t* sizes, int64_t streams, uint8_t* blob,
                                 int64_t blob_bytes, int64_t* offsets, void* stream) {
    if (!scratch || !sizes || !blob || !offsets || streams <= 0 || cap_bytes < 8 || (cap_bytes & 3) || blob_bytes < 0) return MCQ_EINVAL;
    if (((uintptr_t)scratch & 3) || ((uintptr_t)blob & 3)) return MCQ_EINVAL;
    if (streams > 0x7fffffffLL) return MCQ_ETOOLARGE;       // (grid x)
    hipLaunchKernelGGL(rans_scan_kernel, dim3(1), dim3(RANS_SCAN_T), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(sizes),
                       (long long)streams, reinterpret_cast<long long*>(offsets));
    if (mcq_check_launch() != MCQ_OK) return MCQ_ELAUNCH;
    hipLaunchKernelGGL(rans_copy_kernel, dim3((unsigned)streams), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t*>(scratch),
                       (long long)(cap_bytes / 4), reinterpret_cast<const long long*>(sizes), reinterpret_cast<const long long*>(offsets),
                       reinterpret_cast<uint32_t*>(blob), (long long)blob_bytes);
    return mcq_check_launch();
}

extern "C" int mcq_rans_decode_dev(const uint8_t* blob, int64_t blob_bytes, const int64_t* offsets, const uint32_t* const* cdf, const int32_t* m,
                                   const int32_t* k, const int32_t* hw, int32_t levels, int32_t n, int32_t level0, int32_t row_levels,
                                   int64_t* const* codes, int32_t* status, void* stream) {
    if (!blob || !offsets || !cdf || !m || !k || !hw || !codes || !status || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return MCQ_EINVAL;
    if (n <= 0 || level0 < 0 || row_levels < level0 + levels || blob_bytes < 0) return MCQ_EINVAL;
    if (n > 65535) return MCQ_ETOOLARGE;            // (grid y)
    RansDecK q;
    for (int l = 0; l < levels; ++l) {
        if (!codes[l] || !cdf[l] || m[l] <= 0 || k[l] <= 0 || hw[l] <= 0 || k[l] > RANS_KMAX) return MCQ_EINVAL;      // (the table is held in LDS)
        if ((long long)m[l] * hw[l] > MCQ_RANS_DEV_MAX_SYMBOLS) return MCQ_ETOOLARGE;
        q.codes[l] = reinterpret_cast<long long*>(codes[l]); q.cdf[l] = cdf[l];
        q.m[l] = m[l]; q.k[l] = k[l]; q.hw[l] = hw[l];
    }
    q.level0 = level0; q.row_levels = row_levels; q.blob = blob; q.blob_bytes = blob_bytes;
    q.offsets = reinterpret_cast<const long long*>(offsets); q.status = status;
    hipLaunchKernelGGL(rans_decode_kernel, dim3((unsigned)levels, (unsigned)n), dim3(RANS_DEC_T), 0, (hipStream_t)stream, q);
    return mcq_check_launch();
}
