// iwae.hpp -- the K-sample importance-weighted bound on log p(x) (vaeb_marginal_ll,
// include/vaeb_hip.h), with the encoder q(z | x) as the proposal:
//
//   z_k = mu + exp(lv / 2) eps_k,   log w_k = log p(x | z_k) + 1/2 sum_j (eps_kj^2 + lv_j - z_kj^2)
//   IW_K(x) = logsumexp_k log w_k - log K
//
// The encoder and heads run once per chunk (c->mu, c->lv); per stack of S sample planes
//   iw_sample_kernel   eps, z (plane-major, as the decoder phases read it) and the latent term
//   PDecHid, PDecOut   the step's own decoder phases over the S * Mbp stacked rows (phases.hpp):
//                      they leave the per-row log p(x | z) partials lp_part[S * Mbp][nctD]
//   iw_lse_kernel      log w per (plane, row), folded in ascending k into a running
//                      (max, scaled sum) per row; after sample K - 1 the row value
// and iw_sum_kernel adds the chunk's row values to eval_acc[0] in a fixed order.  Samples
// are folded in ascending k whatever S is, so a row's value does not depend on how many
// planes fit in a pass.
#pragma once
#include "kernels_aux.hpp"

namespace vaeb {

struct IwArgs {
    int Z, Mb, Mbp, S, nctD;
    int k0, K;             // this stack holds samples k0 .. k0 + S - 1 of K
    float logK;
    int64_t row0;          // global row of the chunk's row 0 (the Philox counter)
    int eps_mode;          // 0 philox, 1 host buffer
    uint64_t seed;
    const int64_t* step;   // Philox step counter (read only)
    const float* eps_in;   // host mode: sample k, chunk row m at [(k * eps_ld + m) * Z]
    int64_t eps_ld;
    const float *mu, *lv;  // [Mbp][Z]
    float* z;              // [S][Mbp][Z]
    float* lat;            // [S][Mbp] latent term
    const float* lp_part;  // [S][Mbp][nctD]
    float* ms;             // [Mbp][2] running (max, sum of exp(lw - max))
    float* rows;           // [Mb] IW_K per row (written after sample K - 1)
};

// One 16-lane group per (plane, row): lane li takes the latents li, li + 16, ...; pad rows
// are written as z = 0 (PDecHid reads them).  Grid: S * Mbp / 16 workgroups of 256.
__global__ __launch_bounds__(256) void iw_sample_kernel(IwArgs a) {
    const int li = threadIdx.x & 15;
    const int nrb = a.Mbp >> 4;
    const int p = blockIdx.x / nrb;
    const int m = (blockIdx.x % nrb) * 16 + (threadIdx.x >> 4);
    const int k = a.k0 + p;
    const int Z = a.Z;
    const bool valid = m < a.Mb;
    const rsrc_t bmu = mkbuf(a.mu, (int64_t)a.Mbp * Z * 4);
    const rsrc_t blv = mkbuf(a.lv, (int64_t)a.Mbp * Z * 4);
    // the sample's plane of the pushed noise (blockIdx.x, hence k, is workgroup-uniform)
    const rsrc_t be = mkbuf(a.eps_mode == 1 ? a.eps_in + (int64_t)k * a.eps_ld * Z : nullptr,
                            a.eps_mode == 1 ? (int64_t)a.Mb * Z * 4 : 0);
    const int64_t stp = a.step ? *a.step : 0;
    const uint64_t c23 = philox_c23(stp, 1u | ((uint32_t)(k + 1) << 1));
    float* zrow = a.z + ((int64_t)p * a.Mbp + m) * Z;
    float t = 0.f;
    for (int j = li; j < Z; j += 16) {
        const uint32_t o = valid ? (uint32_t)(m * Z + j) * 4u : kOOB;
        const float mu = bld(bmu, o), lv = bld(blv, o);
        float e = 0.f;
        if (valid) e = a.eps_mode == 1 ? bld(be, o) : philox_normal(a.seed, (uint32_t)(a.row0 + m), (uint32_t)j, c23);
        const float z = valid ? mu + fexp(0.5f * lv) * e : 0.f;
        zrow[j] = z;
        t += valid ? e * e + lv - z * z : 0.f;
    }
    t = sum16(t);
    if (li == 0) a.lat[(int64_t)p * a.Mbp + m] = 0.5f * t;
}

// One thread per row: the stack's planes in ascending k.  A non-finite log w poisons the
// row's sum (NaN), never dropped: max() would ignore a NaN and exp() would lose a -inf.
__global__ __launch_bounds__(256) void iw_lse_kernel(IwArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.Mb) return;
    const rsrc_t blp = mkbuf(a.lp_part, (int64_t)a.S * a.Mbp * a.nctD * 4);
    float mx = 0.f, s = 0.f;
    if (a.k0 > 0) { mx = a.ms[2 * i]; s = a.ms[2 * i + 1]; }
    for (int p = 0; p < a.S; ++p) {
        const uint32_t base = (uint32_t)((p * a.Mbp + i) * a.nctD) * 4u;
        double lp = 0;
        for (int t0 = 0; t0 < a.nctD; t0 += 8) {   // fixed order, 8 loads in flight
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = bld(blp, t0 + u < a.nctD ? base + (uint32_t)(t0 + u) * 4u : kOOB);
#pragma unroll
            for (int u = 0; u < 8; ++u) lp += (double)v[u];
        }
        const float lw = (float)(lp + (double)a.lat[(int64_t)p * a.Mbp + i]);
        if (a.k0 + p == 0) {   // the first sample: no -inf - -inf
            mx = lw;
            s = 1.f;
        } else {
            const float m2 = fmaxf(mx, lw);
            s = s * fexp(mx - m2) + fexp(lw - m2);
            mx = m2;
        }
        if (!(fabsf(lw) < __builtin_inff())) s = __builtin_nanf("");
    }
    if (a.k0 + a.S < a.K) {
        a.ms[2 * i] = mx;
        a.ms[2 * i + 1] = s;
    } else {
        a.rows[i] = mx + flog(s) - a.logK;
    }
}

// eval_acc[0] += the chunk's row values, in a fixed order: strided per-thread sums in
// double, a butterfly per wave, then the wave sums in wave order (as elbo_reduce).
__global__ __launch_bounds__(256) void iw_sum_kernel(const float* rows, int64_t n, double* eval_acc) {
    __shared__ double sh[4];
    const double v = block_sum256w(strided_sum<8>(rows, n), sh);
    if (threadIdx.x == 0) eval_acc[0] += v;
}

}  // namespace vaeb
