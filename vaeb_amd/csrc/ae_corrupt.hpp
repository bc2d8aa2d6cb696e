// ae_corrupt.hpp -- input corruption of the layer-stack engine's denoising training
// (include/vaeb_hip.h enum vaeb_ae_corruption; engine_ae.inc ae_corrupt_rows).
//
// A corrupting context's step forms xt [M x D] from the gathered rows X = Xtr[idx] once:
//   MASK         xt = 0 if r < p, else x
//   SALT_PEPPER  xt = 0 if r < p / 2, 1 if p / 2 <= r < p, else x
//   GAUSS        xt = x + p n
// r a uniform on the 2^-24 grid of [0, 1), n a standard normal, p the context's level.  The first
// encoder layer's forward and its weight gradient then read xt ungathered, so both see the same
// bits and each element's Philox block runs once; every other use of x (the output layer's
// observations, the value) keeps the clean rows.  The comparisons are of exactly representable
// float32 values (p / 2 is exact), so a host restatement decides bit-identically.
//
// The draw of element (m, d): rin[m][d] (host mode), or one Philox4x32-10 block at
//   c0 = idx[m] (the dataset row), c1 = 0x80000000 | d, c2, c3 = philox_c23(step, 0)
// with r = (out2 >> 8) / 2^24 and n = philox_normal of that counter (out0, out1).  Bit 31 of c1
// marks input corruption: the latent draws have c1 < 2^30, the FVS weight noise sets bit 30.
#pragma once
#include "ae_mlp.hpp"   // el

namespace vaeb {
namespace ae {

enum : int { CORRUPT_MASK = 1, CORRUPT_SALT_PEPPER = 2, CORRUPT_GAUSS = 3 };   // vaeb_ae_corruption
constexpr uint32_t kCorruptC1 = 0x80000000u;

struct AeCorruptArgs {
    const float* X; int x_rows;   // Xtr [x_rows x D]
    const int* idx;               // [M] dataset rows
    int M, D;
    int kind; float level;
    const float* rin;             // host mode: the draws [M x D] of these rows; nullptr: Philox
    uint64_t seed; int64_t step;
    float* out;                   // xt [M x D]
};

// One thread per element, M * D < 2^31 / 4 (the buffers are below 2 GiB).  A thread past the end
// runs the rounds on row 0 and stores nothing: no lane leaves before the Philox block, the loads
// are masked through their offsets.  Grid: ceil(M * D / 256) workgroups of 256.
__global__ __launch_bounds__(256) void ae_corrupt_kernel(AeCorruptArgs a) {
    const rsrc_t bx = mkbuf(a.X, (int64_t)a.x_rows * a.D * 4);
    const rsrc_t br = mkbuf(a.rin ? a.rin : a.X, (int64_t)(a.rin ? a.M : a.x_rows) * a.D * 4);
    const int total = a.M * a.D;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool ok = i < total;
    const int m = ok ? i / a.D : 0, d = ok ? i - m * a.D : 0;
    const int row = ok ? a.idx[m] : -1;
    const float x = el(bx, a.D, row, d, a.x_rows, a.D);
    const float p = a.level;
    float v;
    if (a.kind == CORRUPT_GAUSS) {
        const float n = a.rin ? el(br, a.D, ok ? m : -1, d, a.M, a.D)
                              : philox_normal(a.seed, (uint32_t)(ok ? row : 0), kCorruptC1 | (uint32_t)d,
                                              philox_c23(a.step, 0u));
        v = x + p * n;
    } else {
        float r;
        if (a.rin) {
            r = el(br, a.D, ok ? m : -1, d, a.M, a.D);
        } else {
            const uint64_t c23 = philox_c23(a.step, 0u);
            uint32_t ctr[4] = {(uint32_t)(ok ? row : 0), kCorruptC1 | (uint32_t)d, (uint32_t)c23, (uint32_t)(c23 >> 32)};
            philox4x32(ctr, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
            r = (float)(ctr[2] >> 8) * (1.0f / 16777216.0f);   // [0, 1), exact
        }
        if (a.kind == CORRUPT_MASK) v = r < p ? 0.f : x;
        else v = r < 0.5f * p ? 0.f : (r < p ? 1.f : x);
    }
    if (ok) a.out[i] = v;
}

}  // namespace ae
}  // namespace vaeb
