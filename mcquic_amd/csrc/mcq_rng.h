// The counter-based generator behind every draw made inside a kernel (the soft assignment's random drop and Gumbel noise,
// vq_train.hip; the training input transform's per-image decisions, augment.hip): ONE definition.
//
// `rng_state` = {seed, offset} (two uint64 in device memory, so that a captured hipGraph sees a fresh offset on every replay).
// u(stream, i) = a 24-bit uniform in [0, 1) from two rounds of a 32-bit avalanche mixer over (seed, offset, stream, element
// index i): any kernel, any thread layout and the backward pass reproduce element i's draw from its index alone.  Not torch's
// Philox stream (no RNG-stream parity is promised by either side: the draws are i.i.d. uniforms); mcq_hash_uniform_f32
// materialises them for tests.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct RngState { uint32_t s0, s1, o0, o1; };
__device__ __forceinline__ RngState rng_load(const unsigned long long* st) {
    RngState r = {0u, 0u, 0u, 0u};
    if (st) {
        const unsigned long long seed = st[0], off = st[1];
        r.s0 = (uint32_t)seed; r.s1 = (uint32_t)(seed >> 32); r.o0 = (uint32_t)off; r.o1 = (uint32_t)(off >> 32);
    }
    return r;
}
__device__ __forceinline__ uint32_t rng_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float rng_uniform(const RngState& r, uint32_t stream, size_t idx) {
    uint32_t h = rng_mix((uint32_t)idx ^ r.s0);
    h = rng_mix(h + (uint32_t)((unsigned long long)idx >> 32) * 0x9E3779B1u + r.s1 + r.o0 * 0x85EBCA77u + r.o1 * 0x27D4EB2Fu + stream * 0xC2B2AE3Du);
    return (float)(h >> 8) * 5.9604644775390625e-08f;            // k / 2^24, k in [0, 2^24): float32's own grid on [0, 1), like torch.rand
}
