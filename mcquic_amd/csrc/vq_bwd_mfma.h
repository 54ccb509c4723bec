// MFMA forms of the soft assignment's two backward contractions (vq_bwd_mfma.hip), dispatched by mcq_vq_soft_bwd_f32 (vq_train.hip).
#pragma once
#include <stdint.h>

struct VqBwdK {
    const float* ddist;      // [rows, k], rows = N m hw ordered (n, g, pixel)
    const float* rowsum;     // [rows]
    const float* x;          // [N, m d, hw]
    const float* xt;         // [N hw, m d]   channel-major copy of x
    const float* dqt;        // [N hw, m d]   channel-major copy of the incoming gradient
    const int64_t* index;    // [rows] sampled codeword
    const float* hot;        // [rows] its straight-through value
    const float* cb;         // [m, k, d]
    float* dx;               // [N, m d, hw]
    float* dcb;              // [m, k, d]
    int N, m, d, hw, k, rows;
};

// Which form takes a shape is decided once, by mcq_vq_soft_bwd_plan (vq_train.hip; include/mcquic_hip.h): the launches below run what
// it says and decide nothing.  VQ_DC_MFMA_WAVES: the vector slices of the d-codebook form -- the plan grants whole vector pairs per slice.
constexpr int VQ_DC_MFMA_WAVES = 8;
void mcq_vq_dc_mfma_launch(const VqBwdK& p, void* stream);
void mcq_vq_dx_mfma_launch(const VqBwdK& p, int split /* workgroups per 32-row tile: 1 or 2 (the plan's dx_split) */, void* stream);
