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
//
// Training on the bound (vaeb_ae_config.iw_samples = K >= 2, engine_ae.inc ae_iw_forward) stacks all K
// planes of the step's M rows in one pass (stacked row g = k * M + m):
//   ae_iw_sample_kernel      its training form (AeIwArgs.idx set): c0 and yrow from the index
//                            list, the training domain k << 1
//   ae_iw_weight_kernel      per row m the normalised weights wn_k = w_k / sum_k' w_k', the row
//                            value, and the output deltas of stacked row g scaled by wn_k; the
//                            backward below the output layer is linear in those deltas
//   PAeBwd B_LATENT_IW       (ae_mlp.hpp) dmu_k, dlv_k per stacked row
//   ae_iw_plane_sum_kernel   dmu[m] = sum_k dmu_k, dlv[m] = sum_k dlv_k, ascending k
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
    float* lat;            // [S * R] latent term 1/2 sum_j (eps^2 + lv - z^2) (two-mode prior: below)
    int* yrow;             // [S * R] the row of the chunk's x each stacked row observes
    const int* idx;        // training form: the dataset rows [R] of the step (c0 and yrow), the
                           // training domain k << 1, row0 = the step's offset in the call's idx
                           // list of n rows; nullptr: the evaluation form
};

// One 16-lane group per (plane, row): lane li takes the latents li, li + 16, ...  No pad
// rows: the layer-stack kernels bound-check rows themselves.  Grid: ceil(S * R / 16)
// workgroups of 256.
// The body is shared by the kernel of the N(0, 1) prior and that of the two-mode prior (TM,
// ae_mlp.hpp AePriorArgs: lat = sum_j [1/2 eps^2 + 1/2 lv + log p(z) + 1/2 log 2 pi]); the prior's
// arguments exist in the latter alone.
template <bool TM>
DEV void ae_iw_sample_body(const AeIwArgs& a, const AePriorArgs<TM>& pr) {
    const int li = threadIdx.x & 15;
    const int g = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (g >= a.S * a.R) return;   // whole 16-lane groups leave; sum16 stays inside a group
    const int p = g / a.R, m = g - p * a.R;
    const int k = a.k0 + p;
    const int Dz = a.Dz;
    const uint64_t c23 = philox_c23(a.step, a.idx ? (uint32_t)k << 1 : 1u | ((uint32_t)(k + 1) << 1));
    const int xrow = a.idx ? a.idx[m] : m;
    const uint32_t c0 = a.idx ? (uint32_t)xrow : (uint32_t)(a.row0 + m);
    const float* erow = a.eps_mode == 1 ? a.eps_in + ((int64_t)k * a.n + a.row0 + m) * Dz : nullptr;
    const float* mrow = a.mu + (int64_t)m * Dz;
    const float* vrow = a.lv + (int64_t)m * Dz;
    float* zrow = a.z + (int64_t)g * Dz;
    float t = 0.f;
    for (int j = li; j < Dz; j += 16) {
        const float mu = mrow[j], lv = vrow[j];
        const float e = erow ? erow[j] : philox_normal(a.seed, c0, (uint32_t)j, c23);
        const float z = mu + fexp(0.5f * lv) * e;
        zrow[j] = z;
        if constexpr (TM) t += 0.5f * (e * e + lv) + pr.logp(z);
        else t += e * e + lv - z * z;
    }
    t = sum16(t);
    if (li == 0) {
        a.lat[g] = TM ? t : 0.5f * t;
        a.yrow[g] = xrow;
    }
}
__global__ __launch_bounds__(256) void ae_iw_sample_kernel(AeIwArgs a) { ae_iw_sample_body<false>(a, AePriorArgs<false>{}); }
__global__ __launch_bounds__(256) void ae_iw_sample_tm_kernel(AeIwArgs a, AePriorArgs<true> pr) {
    ae_iw_sample_body<true>(a, pr);
}

struct AeIwWeightArgs {
    int M, K, D, nct;      // rows per plane, planes, output width, log-lik partials per stacked row
    double logK;
    const float* llpart;   // [K * M][nct] log p(x | z_k) partials of the output layer
    const float* lat;      // [K * M] latent terms
    double* lw;            // [K * M] scratch: log w, then exp(log w - max)
    float* wt;             // [K * M] normalised weights
    float* rowval;         // [M] max + log sum - log K
    float *dA, *dA2;       // [K * M][D] output deltas, scaled in place (dA2: cont output, or nullptr)
};

// Fixed-order sum over the 256 threads of a workgroup (LDS tree); every thread gets the result.
DEV double iw_block_sum(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// One workgroup of 256 per row m.  log w_k: one 16-lane group per plane (k = group, group + 16,
// ...), lane li adds the row's partials li, li + 16, ... in fp64, a 16-lane butterfly in fp64 (a
// fixed order; every lane of the group ends with the same bits), then the latent term.  At
// Dobs = 784, log w ~ -540: a float32 sum would put ~1e-4 of absolute error one-to-one into wn;
// the max and the differences log w_k - max stay in fp64 too.  A non-finite log w_k makes the
// row's value and weights NaN (never dropped: max() would ignore a NaN and exp() would lose a
// -inf).  Scaling: one wave per plane, lanes along the row.
__global__ __launch_bounds__(256) void ae_iw_weight_kernel(AeIwWeightArgs a) {
    __shared__ double sh[256];
    const int m = blockIdx.x, t = threadIdx.x;
    const int li = t & 15;
    double mx = -__builtin_inf();
    bool bad = false;
    for (int k = t >> 4; k < a.K; k += 16) {
        const int64_t g = (int64_t)k * a.M + m;
        const float* part = a.llpart + g * a.nct;
        double lp = 0.0;
        for (int c = li; c < a.nct; c += 16) lp += (double)part[c];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) lp += __shfl_xor(lp, o, 16);
        lp += (double)a.lat[g];
        if (li == 0) a.lw[g] = lp;
        if (!(fabs(lp) < __builtin_inf())) bad = true;
        mx = fmax(mx, lp);
    }
    // max is exact in any order
    sh[t] = bad ? __builtin_nan("") : mx;
    __syncthreads();   // also: lw of the row's planes, written above by other threads
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            const double x = sh[t], y = sh[t + o];
            sh[t] = (x != x || y != y) ? __builtin_nan("") : fmax(x, y);
        }
        __syncthreads();
    }
    mx = sh[0];   // NaN: some log w of the row is not finite
    double s = 0.0;
    for (int k = t; k < a.K; k += 256) {
        const int64_t g = (int64_t)k * a.M + m;
        const double e = exp(a.lw[g] - mx);
        a.lw[g] = e;
        s += e;
    }
    s = iw_block_sum(s, sh);
    if (t == 0) a.rowval[m] = (float)(mx + log(s) - a.logK);
    const double inv = 1.0 / s;
    for (int k = t; k < a.K; k += 256) {
        const int64_t g = (int64_t)k * a.M + m;
        a.wt[g] = (float)(a.lw[g] * inv);
    }
    __syncthreads();   // wt of the row's planes: written above by other threads of this workgroup
    const int lane = t & 63;
    for (int k = t >> 6; k < a.K; k += 4) {
        const int64_t g = (int64_t)k * a.M + m;
        const float w = a.wt[g];
        float* r1 = a.dA + g * a.D;
        for (int n = lane; n < a.D; n += 64) r1[n] *= w;
        if (a.dA2) {
            float* r2 = a.dA2 + g * a.D;
            for (int n = lane; n < a.D; n += 64) r2[n] *= w;
        }
    }
}

// d [K * M][Dz] -> rows [0, M): d[m][j] = sum_k d[k * M + m][j] in ascending k, in place, for
// the two arrays (dmu, dlv).  One thread per (m, j): it reads and writes its own elements only.
__global__ __launch_bounds__(256) void ae_iw_plane_sum_kernel(float* d1, float* d2, int M, int Dz, int K) {
    const int64_t n = (int64_t)M * Dz;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s1 = d1[i], s2 = d2[i];
    for (int k = 1; k < K; ++k) {
        s1 += d1[(int64_t)k * n + i];
        s2 += d2[(int64_t)k * n + i];
    }
    d1[i] = s1;
    d2[i] = s2;
}

}  // namespace ae
}  // namespace vaeb
