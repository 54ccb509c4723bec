// Sizes of the packed operand streams of the convolution kernels: what conv_pack.hip writes and conv_launch.hip reads.
#pragma once
#include <stddef.h>

constexpr int MCQ_TAIL_STEPS = 32;       // (16 until ABI 8: the four-tap walk's weight ring runs 8 LIVE steps = up to 26 dense steps ahead)
constexpr int H16_TAIL_STEPS = 16;       // conv_head16.h: zero steps after the last k-step (the weight ring over-reads H16_PFA of them)

inline bool head16_shape(int Cout, int ksize) { return Cout <= 16 && ksize == 3; }
inline size_t head16_floats(int Cin) { return ((size_t)((Cin + 3) / 4) * 9 + H16_TAIL_STEPS) * 64; }

inline bool t16_shape(int Cout, int Cin, int ksize) { return ksize == 3 && Cout >= 32 && Cout % 16 == 0 && (Cin == 64 || Cin == 128); }
inline size_t t16_floats(int Cout, int Cin, int ksize) { return t16_shape(Cout, Cin, ksize) ? (size_t)(Cout / 16) * (size_t)(Cin / 4) * 9 * 64 : 0; }

inline int pairs_padded(int Cin, int ks) {        // 1x1 loops advance a whole prefetch ring (<= 16 pairs) at a time
    const int S = (Cin + 1) / 2;
    return ks == 1 ? (S + 15) & ~15 : S;
}
inline int steps_padded(int Cin, int ks) { return pairs_padded(Cin, ks) * ks * ks; }
// The operand stream of conv_mfma_kernel exists once per tile height: 128-, 64- and 32-row copies, each with its own
// zero steps for the prefetch tail (MCQ_TAIL_STEPS: the deepest weight ring of any instance); layers conv_t16.h can take carry a
// fourth section in its order.
inline size_t section_floats(int Cout, int Cin, int ks, int bands) {
    const size_t ntile = (size_t)(Cout + 32 * bands - 1) / (32 * bands);
    return (ntile * (size_t)steps_padded(Cin, ks) + MCQ_TAIL_STEPS) * 64 * bands;
}

inline size_t general_floats(int Cout, int Cin, int ks) {
    return section_floats(Cout, Cin, ks, 4) + section_floats(Cout, Cin, ks, 2) + section_floats(Cout, Cin, ks, 1) + t16_floats(Cout, Cin, ks);
}

inline size_t wino_section_floats(int Cout, int Cin, int bands) {
    const size_t ntile = (size_t)(Cout + 32 * bands - 1) / (32 * bands);
    return (ntile * (size_t)((Cin + 1) / 2) * 12 + 16) * 64 * bands;
}

inline size_t wino2d_floats(int Cout, int Cin) {           // [Cout/32][Cin/2 x 16 (+ 16 tail)][64 lanes]
    return (((size_t)(Cout + 31) / 32) * (size_t)((Cin + 1) / 2) * 16 + 16) * 64;
}
