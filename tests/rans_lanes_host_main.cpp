// Stand-alone host build of the lanes coder (mcquic_amd/csrc/rans.cpp) for tests/test_rans_lanes_host.py: no HIP, no library.
// Round-trips mcq_rans_lanes_encode_batch / mcq_rans_lanes_decode_batch over every width and a few lengths, then feeds the decoder the
// malformed streams of the layout's list; prints "ok <streams> <refusals>" and returns 0, or says what went wrong and returns 1.
// This is the program to build with -fsanitize=address,undefined: every buffer below is sized exactly, so a read or write past a
// stream, a table or an output row is reported.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../mcquic_amd/csrc/rans.cpp"

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int fail(const char* what, int a = 0, int b = 0) { printf("FAILED: %s (%d, %d)\n", what, a, b); return 1; }

int main() {
    const int k = 512, m = 3, streams = 3;
    // group 0 uniform, group 1 one wide symbol and width 1 elsewhere, group 2 alternating widths
    std::vector<uint32_t> cdf((size_t)m * (k + 1));
    for (int g = 0; g < m; ++g) {
        uint32_t* t = cdf.data() + (size_t)g * (k + 1);
        t[0] = 0;
        for (int i = 0; i < k; ++i) {
            uint32_t w = 128;
            if (g == 1) w = i == 7 ? 65536u - (k - 1) : 1u;
            if (g == 2) w = i % 2 ? 1u : 255u;
            t[i + 1] = t[i] + w;
        }
        if (t[k] != 65536u) return fail("table total", g);
    }
    const int widths[] = {0, 1, 2, 4, 8, 16, 32, 64};
    const int lengths[] = {1, 3, 63, 64, 65, 129, 700};
    int coded = 0, refused = 0;
    std::vector<uint8_t> keep;                      // one stream with renormalisation words, for the malformed cases
    int64_t keep_hw = 0;
    for (int W : widths)
        for (int hw : lengths) {
            const int64_t n = (int64_t)m * hw;
            const int64_t stride = 4 * (1 + 2 * (W ? W : 64) + n);
            std::vector<int32_t> sym((size_t)(streams * n)), back((size_t)(streams * n), -1);
            for (auto& v : sym) v = (int32_t)(rnd() % k);
            std::vector<uint8_t> out((size_t)(streams * stride));
            std::vector<int64_t> sizes(streams), offs(streams + 1, 0);
            if (mcq_rans_lanes_encode_batch(sym.data(), streams, m, hw, cdf.data(), k, W, out.data(), stride, sizes.data(), 2) != MCQ_OK)
                return fail("encode", W, hw);
            std::vector<uint8_t> blob;
            for (int i = 0; i < streams; ++i) {
                if (sizes[i] < 4 * (1 + 2 * (W ? W : 1)) || sizes[i] > stride || (sizes[i] & 3)) return fail("size", W, hw);
                blob.insert(blob.end(), out.begin() + i * stride, out.begin() + i * stride + sizes[i]);
                offs[i + 1] = offs[i] + sizes[i];
            }
            if (mcq_rans_lanes_decode_batch(blob.data(), (int64_t)blob.size(), offs.data(), streams, m, hw, cdf.data(), k, back.data(), 2) != MCQ_OK)
                return fail("decode", W, hw);
            if (back != sym) return fail("round trip", W, hw);
            coded += streams;
            if (W == 4 && hw == 700) { keep.assign(blob.begin(), blob.begin() + sizes[0]); keep_hw = hw; }
        }
    if (keep.size() <= 4 * (1 + 2 * 4)) return fail("the kept stream holds no words");

    auto refuses = [&](const std::vector<uint8_t>& s, int64_t a, int64_t b, int64_t blob_bytes) {
        std::vector<int32_t> back((size_t)(m * keep_hw), 7);
        std::vector<uint8_t> exact(s);              // sized exactly: a read past the stream is a heap overflow
        if (exact.empty()) exact.push_back(0);
        const int64_t offs[2] = {a, b};
        const int rc = mcq_rans_lanes_decode_batch(exact.data(), blob_bytes, offs, 1, m, keep_hw, cdf.data(), k, back.data(), 1);
        for (int32_t v : back) if (v != 0) return false;
        return rc == MCQ_EINVAL;
    };
    const int64_t len = (int64_t)keep.size();
    std::vector<uint8_t> s;
    s = keep; s[0] = 'X';                                    if (!refuses(s, 0, len, len)) return fail("wrong prefix"); ++refused;
    s = keep; s[3] = 3;                                      if (!refuses(s, 0, len, len)) return fail("W = 3"); ++refused;
    s = keep; s[3] = 0;                                      if (!refuses(s, 0, len, len)) return fail("W = 0"); ++refused;
    s = keep; s[3] = 128;                                    if (!refuses(s, 0, len, len)) return fail("W = 128"); ++refused;
    s.assign(keep.begin(), keep.begin() + 4 * (1 + 2 * 4) - 4); if (!refuses(s, 0, (int64_t)s.size(), (int64_t)s.size())) return fail("short head"); ++refused;
    s.assign(keep.begin(), keep.begin() + 4);                if (!refuses(s, 0, 4, 4)) return fail("prefix only"); ++refused;
    s.clear();                                               if (!refuses(s, 0, 0, 0)) return fail("empty"); ++refused;
    s.assign(keep.begin(), keep.end() - 1);                  if (!refuses(s, 0, len - 1, len - 1)) return fail("length % 4"); ++refused;
    s.assign(keep.begin(), keep.end() - 4);                  if (!refuses(s, 0, len - 4, len - 4)) return fail("out of words"); ++refused;
    s = keep;                                                if (!refuses(s, 0, len + 4, len)) return fail("past the blob"); ++refused;
    s = keep;                                                if (!refuses(s, 8, 4, len)) return fail("decreasing"); ++refused;
    s = keep;                                                if (!refuses(s, -4, len, len)) return fail("negative"); ++refused;
    {   // a table whose first entry is not 0: the bin the bisection ends in does not contain cum
        std::vector<int32_t> sym((size_t)(m * 5), 0), back((size_t)(m * 5), 7);
        std::vector<uint8_t> out(4 * (1 + 2 * 2 + m * 5));
        int64_t size = -1;
        if (mcq_rans_lanes_encode_batch(sym.data(), 1, m, 5, cdf.data(), k, 2, out.data(), (int64_t)out.size(), &size, 1) != MCQ_OK) return fail("encode zeros");
        std::vector<uint32_t> broken(cdf);
        broken[0] = 65535u;
        const int64_t offs[2] = {0, size};
        const int rc = mcq_rans_lanes_decode_batch(out.data(), size, offs, 1, m, 5, broken.data(), k, back.data(), 1);
        if (rc != MCQ_EINVAL) return fail("broken table", rc);
        for (int32_t v : back) if (v != 0) return fail("broken table: zeros");
        ++refused;
    }
    {   // a code outside [0, k) and an empty bin are refused by the encoder before anything is indexed
        std::vector<int32_t> sym((size_t)(m * 5), 1);
        std::vector<uint8_t> out(4 * (1 + 2 * 64 + m * 5));
        int64_t size = -1;
        sym[7] = k;
        if (mcq_rans_lanes_encode_batch(sym.data(), 1, m, 5, cdf.data(), k, 2, out.data(), (int64_t)out.size(), &size, 1) != MCQ_EINVAL || size != 0) return fail("code k");
        sym[7] = -1;
        if (mcq_rans_lanes_encode_batch(sym.data(), 1, m, 5, cdf.data(), k, 2, out.data(), (int64_t)out.size(), &size, 1) != MCQ_EINVAL) return fail("code -1");
        sym[7] = 1;
        if (mcq_rans_lanes_encode_batch(sym.data(), 1, m, 5, cdf.data(), k, 3, out.data(), (int64_t)out.size(), &size, 1) != MCQ_EINVAL) return fail("lanes = 3");
        refused += 3;
    }
    printf("ok %d %d\n", coded, refused);
    return 0;
}
