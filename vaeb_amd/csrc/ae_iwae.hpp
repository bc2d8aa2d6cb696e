// ae_iwae.hpp -- the K-sample importance-weighted bound on log p(x) of the layer-stack
// engine's Gaussian latent (vaeb_ae_marginal_ll, include/vaeb_hip.h); the quantity and the
// fold are iwae.hpp's, the network is ae_mlp.hpp's.
//
// The encoder runs once per chunk of R rows (mu, lv).  Per pass of S stacked sample planes
//   ae_iw_sample_kernel   eps, z at stacked row p * R + m, the latent term and the gather
//                         list yrow[p * R + m] = m (every plane reads the chunk's x)
//   PAeFwd                the decoder layers over the S * R stacked rows, then the output
//                         layer in its value-only form (Y set, dA == nullptr): the per-row
//                         log p(x | z) partials and no store of predictions or deltas
//   iw_lse_kernel         iwae.hpp's fold as it stands (plane stride Mbp = R)
// and iw_sum_kernel adds the chunk's row values in a fixed order.
#pragma once
#include "iwae.hpp"

namespace vaeb {
namespace ae {

struct AeIwArgs {
    int Dz, R, S;          // R rows per plane, S planes in this pass
    int k0;                // the pass holds samples k0 .. k0 + S - 1
    int64_t row0;          // index of the chunk's row 0 in the call's x (the Philox c0)
    int64_t n;             // rows of the call's x (host eps: sample k, row i at row k * n + i)
    int eps_mode;          // 0 philox, 1 host buffer
    uint64_t seed;
    int64_t step;
    const float* eps_in;   // the pushed eps [n * K][Dz]
    const float *mu, *lv;  // [R][Dz]
    float* z;              // [S * R][Dz]
    float* lat;            // [S * R] latent term 1/2 sum_j (eps^2 + lv - z^2)
    int* yrow;             // [S * R] the row of the chunk's x each stacked row observes
};

// One 16-lane group per (plane, row): lane li takes the latents li, li + 16, ...  No pad
// rows: the layer-stack kernels bound-check rows themselves.  Grid: ceil(S * R / 16)
// workgroups of 256.
__global__ __launch_bounds__(256) void ae_iw_sample_kernel(AeIwArgs a) {
    const int li = threadIdx.x & 15;
    const int g = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (g >= a.S * a.R) return;   // whole 16-lane groups leave; sum16 stays inside a group
    const int p = g / a.R, m = g - p * a.R;
    const int k = a.k0 + p;
    const int Dz = a.Dz;
    const uint64_t c23 = philox_c23(a.step, 1u | ((uint32_t)(k + 1) << 1));
    const float* erow = a.eps_mode == 1 ? a.eps_in + ((int64_t)k * a.n + a.row0 + m) * Dz : nullptr;
    const float* mrow = a.mu + (int64_t)m * Dz;
    const float* vrow = a.lv + (int64_t)m * Dz;
    float* zrow = a.z + (int64_t)g * Dz;
    float t = 0.f;
    for (int j = li; j < Dz; j += 16) {
        const float mu = mrow[j], lv = vrow[j];
        const float e = erow ? erow[j] : philox_normal(a.seed, (uint32_t)(a.row0 + m), (uint32_t)j, c23);
        const float z = mu + fexp(0.5f * lv) * e;
        zrow[j] = z;
        t += e * e + lv - z * z;
    }
    t = sum16(t);
    if (li == 0) {
        a.lat[g] = 0.5f * t;
        a.yrow[g] = m;
    }
}

}  // namespace ae
}  // namespace vaeb
