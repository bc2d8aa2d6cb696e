// clf_softmax.hpp -- the device code the softmax MLP classifier (include/vaeb_hip.h vaeb_clf_*,
// engine_clf.inc; the reference's degenerate-vae/mlp.py:104-153, 263-329) adds to the layer-stack
// kernels of ae_mlp.hpp.  The hidden layers, the logits (F_LINEAR), the data backward (B_DACT) and
// the weight gradient + update (PAeWgradT<RULE, MASK>) are that file's; new here:
//
//   clf_softmax_kernel   one wavefront per row of the logits a [M x D] (written by the F_LINEAR
//                        forward): e = exp(a - max), P = e / sum e, the row's log-likelihood and the
//                        delta d = dloglik / da.  The output's normalisation spans the row, which no
//                        16-column epilogue tile can see, hence a kernel of its own.
//       Bernoulli (mlp.py:112 on logpdf.py:16-17, 84-87):
//                        ll = sum_j y log(P + 1e-7) + (1 - y) log(1 - P + 1e-7),
//                        dP_j = y_j / (P_j + 1e-7) - (1 - y_j) / (1 - P_j + 1e-7),
//                        d_i = P_i (dP_i - sum_j P_j dP_j)
//       categorical:     ll = sum_j y_j (a_j - max - log sum e),  d_i = y_i - P_i sum_j y_j
//     Lane l owns the columns l, l + 64, ...; the three row reductions (max, sum e, and the pair
//     ll | sum_j P_j dP_j) are DPP adds inside each 16-lane row (sum16's pattern) and two lane
//     exchanges across the four rows: no LDS array, no per-element round trip.
//     A row of D <= 64 kRegCols = 256 columns stays in registers (a, y and e: 12 VGPRs per lane,
//     far from any occupancy step of a 256-thread block);
//     256 covers every class count the reference uses (10) with room to spare, and four columns
//     per lane is where the unrolled loops stop paying for themselves.  A wider row loops over the
//     logits in memory, one pass per reduction, recomputing e (the logits of a row are
//     L2-resident: the forward has just written them).
//     Modes, as the output layer of ae_mlp.hpp has them: predictions only (Y == nullptr), value
//     only (Y, no d), value + P + deltas (Y, P, d).  Row values go to rowval [M]; the step's value
//     is the fixed-order fp64 sum of that array (ae_loglik_kernel, iw_sum_kernel).
//     Monte-Carlo prediction: with Pacc set the kernel adds its P to Pacc (first draw: stores it;
//     last draw: scales the sum by 1 / L), one lane per element, draws in stream order.
//   clf_mask_kernel      weight dropout: theta~ = theta * m over the flat arena, m the byte mask.
//     Parameter i takes output word i & 3 of the Philox4x32-10 block at the counter
//     (c0 = i >> 2, c1 = 0x40000000, c2, c3 = philox_c23(step, domain)) under the context's seed and
//     is kept iff word < T, T = floor(keep 2^32) from the host (64 bits: keep = 1 keeps all).
//   clf_hit_kernel       per row the arg-max of P (the lowest index among equals, as numpy.argmax)
//                        and hit[m] = (Y[m][argmax] == 1) (mlp.py:367-373), one wavefront per row
//   clf_count_kernel     one block adds a chunk's hits to the call's integer count: no atomics
#pragma once
#include "tile_engine.hpp"

namespace vaeb {
namespace clf {

enum : int { LOSS_BERNOULLI = 0, LOSS_CATEGORICAL = 1 };
constexpr int kRegCols = 4;        // columns per lane held in registers: D <= 256
constexpr float kEpsLog = 1e-7f;   // logpdf.py:86

// ---------------------------------------------------------------- 64-lane reductions
// Every lane ends with the same value.  Inside a 16-lane row: the four DPP steps of sum16; across
// the four rows: lane ^ 16 and lane ^ 32.
DEV float max16(float v) {
    v = fmaxf(v, dppf<0xB1>(v));
    v = fmaxf(v, dppf<0x4E>(v));
    v = fmaxf(v, dppf<0x141>(v));
    v = fmaxf(v, dppf<0x140>(v));
    return v;
}
DEV float sum64(float v) {
    v = sum16(v);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
DEV float max64(float v) {
    v = max16(v);
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}

struct SoftmaxArgs {
    const float* a; int M, D;                    // logits [M x D]
    const float* Y; const int* yidx;             // targets, row m at Y[yidx ? yidx[m] : m] (ld D); nullptr: predictions only
    int loss;
    float* P;                                    // predictions [M x D], or nullptr
    float* d;                                    // deltas [M x D], or nullptr
    float* rowval;                               // [M] (with Y)
    float* Pacc; int first, last; float invL;    // Monte-Carlo mean over draws, or nullptr
};

DEV float bern_ll(float y, float P) { return y * flog(P + kEpsLog) + (1.f - y) * flog(1.f - P + kEpsLog); }
DEV float bern_dP(float y, float P) { return y * frcp(P + kEpsLog) - (1.f - y) * frcp(1.f - P + kEpsLog); }

// One row on one wavefront.  REG: the row's a, y and e in registers (D <= 64 kRegCols); otherwise
// every pass reads the logits again.  Columns past D read a = -inf (e = 0) and y = 0.
template <bool REG>
DEV void softmax_row(const SoftmaxArgs& q, int m, int lane) {
    const int D = q.D;
    const int T = REG ? kRegCols : (D + 63) >> 6;
    const float* arow = q.a + (int64_t)m * D;
    const bool obs = q.Y != nullptr;
    const float* yrow = obs ? q.Y + (int64_t)(q.yidx ? q.yidx[m] : m) * D : arow;
    float av[kRegCols], yv[kRegCols], ev[kRegCols];
    if constexpr (REG) {
#pragma unroll
        for (int t = 0; t < kRegCols; ++t) {
            const int j = lane + 64 * t;
            av[t] = j < D ? arow[j] : -INFINITY;
            yv[t] = (obs && j < D) ? yrow[j] : 0.f;
        }
    }
    auto a_at = [&](int t, int j) -> float {
        if constexpr (REG) return av[t];
        else return j < D ? arow[j] : -INFINITY;
    };
    auto y_at = [&](int t, int j) -> float {
        if constexpr (REG) return yv[t];
        else return (obs && j < D) ? yrow[j] : 0.f;
    };
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < T; ++t) mx = fmaxf(mx, a_at(t, lane + 64 * t));
    mx = max64(mx);
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float e = fexp(a_at(t, lane + 64 * t) - mx);
        if constexpr (REG) ev[t] = e;
        s += e;
    }
    const float S = sum64(s), inv = frcp(S);
    auto p_at = [&](int t, int j) -> float {
        if constexpr (REG) return ev[t] * inv;
        else return fexp(a_at(t, j) - mx) * inv;
    };
    const bool bern = q.loss == LOSS_BERNOULLI;
    float dot = 0.f;   // Bernoulli: sum_j P_j dP_j; categorical: sum_j y_j
    if (obs) {
        float ll = 0.f;
        const float logS = flog(S);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int j = lane + 64 * t;
            if (j >= D) continue;
            const float y = y_at(t, j);
            if (bern) {
                const float P = p_at(t, j);
                ll += bern_ll(y, P);
                if (q.d) dot += P * bern_dP(y, P);
            } else {
                ll += y * (a_at(t, j) - mx - logS);
                dot += y;
            }
        }
        ll = sum64(ll);
        if (q.d) dot = sum64(dot);
        if (lane == 0) q.rowval[m] = ll;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int j = lane + 64 * t;
        if (j >= D) continue;
        const int64_t o = (int64_t)m * D + j;
        const float P = p_at(t, j);
        if (q.P) q.P[o] = P;
        if (q.Pacc) {
            float v = q.first ? P : q.Pacc[o] + P;
            if (q.last) v *= q.invL;
            q.Pacc[o] = v;
        }
        if (q.d) {
            const float y = y_at(t, j);
            q.d[o] = bern ? P * (bern_dP(y, P) - dot) : y - P * dot;
        }
    }
}

// Grid: ceil(M / 4) blocks of 4 wavefronts, one row each.
__global__ __launch_bounds__(256) void clf_softmax_kernel(SoftmaxArgs q) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= q.M) return;   // the whole wavefront
    if (q.D <= 64 * kRegCols) softmax_row<true>(q, m, lane);
    else softmax_row<false>(q, m, lane);
}

// ---------------------------------------------------------------- weight dropout
struct MaskArgs {
    const float* theta; float* thm; uint8_t* mask;   // thm / mask: either may be nullptr
    int64_t P;
    uint64_t seed; int64_t step; uint32_t domain;
    uint64_t T;                                      // keep iff word < T
};

// One thread per group of four parameters (one Philox block).  The arenas come from hipMalloc
// (256-byte aligned), so a whole group is one 16-byte load and store and one 4-byte mask store.
__global__ __launch_bounds__(256) void clf_mask_kernel(MaskArgs q) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x, i0 = 4 * g;
    if (i0 >= q.P) return;
    const uint64_t c23 = philox_c23(q.step, q.domain);
    uint32_t ctr[4] = {(uint32_t)g, 0x40000000u, (uint32_t)c23, (uint32_t)(c23 >> 32)};
    philox4x32(ctr, (uint32_t)q.seed, (uint32_t)(q.seed >> 32));
    bool k[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) k[w] = (uint64_t)ctr[w] < q.T;
    if (i0 + 4 <= q.P) {
        if (q.thm) {
            f32x4 v = *reinterpret_cast<const f32x4*>(q.theta + i0);
            v.x = k[0] ? v.x : 0.f; v.y = k[1] ? v.y : 0.f; v.z = k[2] ? v.z : 0.f; v.w = k[3] ? v.w : 0.f;
            *reinterpret_cast<f32x4*>(q.thm + i0) = v;
        }
        if (q.mask)
            *reinterpret_cast<uint32_t*>(q.mask + i0) =
                (uint32_t)k[0] | (uint32_t)k[1] << 8 | (uint32_t)k[2] << 16 | (uint32_t)k[3] << 24;
        return;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {   // the arena's last, partial group
        if (i0 + w >= q.P) break;
        if (q.thm) q.thm[i0 + w] = k[w] ? q.theta[i0 + w] : 0.f;
        if (q.mask) q.mask[i0 + w] = k[w] ? 1 : 0;
    }
}

// ---------------------------------------------------------------- accuracy
// hit[m] = (Y[m][argmax_j P[m][j]] == 1).  A lane scans its columns in ascending order (a strict >
// keeps the lowest index), then the 64 candidates are folded pairwise: the larger P wins, equal P
// the lower index.
__global__ __launch_bounds__(256) void clf_hit_kernel(const float* P, const float* Y, int M, int D, int* hit) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const float* prow = P + (int64_t)m * D;
    float bv = -INFINITY;
    int bi = 0x7FFFFFFF;
    for (int j = lane; j < D; j += 64) {
        const float v = prow[j];
        if (v > bv || bi == 0x7FFFFFFF) { bv = v; bi = j; }
    }
    for (int o = 1; o < 64; o <<= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) hit[m] = (bi < D && Y[(int64_t)m * D + bi] == 1.0f) ? 1 : 0;
}

// *count += sum of hit[0 .. M): one block, integer adds in a fixed tree.
__global__ __launch_bounds__(256) void clf_count_kernel(const int* hit, int M, long long* count) {
    __shared__ int sh[256];
    int s = 0;
    for (int i = threadIdx.x; i < M; i += 256) s += hit[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count += sh[0];
}

}  // namespace clf
}  // namespace vaeb
