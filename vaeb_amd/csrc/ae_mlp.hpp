// ae_mlp.hpp -- fp32 MFMA layer-stack kernels for the degenerate-vae deterministic
// autoencoder (/root/reference/degenerate-vae/ae.py:41-117, mlp.py:36-91, logpdf.py:46-114,
// infalg.py:148-164), on the same tile engine as the VAEB step (tile_engine.hpp).
//
// One training call train(idx) (ae.py:82-89) on the gathered rows X = Xtr[idx]:
//   forward, per layer:   out = f(in W + b)            PAeFwd (mode ACT / LINEAR)
//                         Z layer linear (ae.py:49)
//   output (ae.py:58-73): binary  P = sigmoid(a), loglik += Y log(P+1e-7) + (1-Y) log(1-P+1e-7)
//                         cont    mu = sigmoid(a_mu), ls2 = a_ls2,
//                                 loglik += -1/2 (log 2 pi + ls2 + (Y-mu)^2 e^-ls2)
//                         fused with the output deltas dlogjoint/da     PAeFwd (mode OUT_*)
//   squared-error output (VAEB_AE_SE, vanilla-ae/ae.py:63-72; vaeb_ae_sq_error on any context):
//                         P = sigmoid(a), se += (Y - P)^2 (kept positive: the step's value is
//                         se / M), delta d(-se)/da = 2 (Y - P) P (1 - P)  PAeFwdT<true> (mode OUT_SE)
//   backward, per layer:  din = (dout W^T) * f'(h)      PAeBwd (mode DACT)
//                         dZ  = dout W^T - Z            PAeBwd (mode ZPRIOR: N(0,1) prior on Z)
//   activated latent (VAEB_AE_LATENT_ACT, vanilla-ae/ae.py:55): Z = f(H Wz + bz) through mode ACT,
//                         dZ = (dout W^T) * f'(Z) through mode DACT with h = Z; no prior on Z
//   Gaussian latent (VAEB_AE_LATENT_GAUSS; replaces the linear Z layer and its prior):
//                         mu = H Wzmu + bzmu, lv = H Wzlv + bzlv, z = mu + exp(lv/2) eps,
//                         -KL partials 1/2 (1 + lv - mu^2 - e^lv)      PAeFwd (mode LATENT, 2 heads)
//                         dz = dout W^T, dmu = dz - mu,
//                         dlv = 1/2 dz (z - mu) + 1/2 (1 - e^lv)       PAeBwd (mode LATENT)
//   importance-weighted training (iw_samples = K >= 2, ae_iwae.hpp): the decoder on K M stacked
//                         rows, output deltas scaled by the normalised weights wn, then
//                         dmu_k = dz - wn z, dlv_k = 1/2 (dz - wn z)(z - mu) + 1/2 wn
//                                                               PAeBwdT<true> (mode LATENT_IW)
//   two-mode latent prior (VAEB_AE_PRIOR_TWO_MODE, Gaussian latent only): per latent dimension
//                         p(z) = 1/2 N(z; 0, s^2) + 1/2 N(z; a, s^2); with c = 1 / s^2,
//                         t = a (2 z - a) c / 2, r = sigmoid(t),
//                         log p(z) = -1/2 log 2 pi - log(2 s) - 1/2 c z^2 + softplus(t),
//                         dlog p / dz = -c (z - a r).  The KL has no closed form: the latent
//                         partials are 1/2 (1 + lv) - log(2 s) - 1/2 c z^2 + softplus(t) at the
//                         step's z                          PAeFwdT<false, true> (mode LATENT)
//                         g = dz - c (z - a r), dmu = g, dlv = 1/2 g (z - mu) + 1/2
//                                                           PAeBwdT<false, true> (mode LATENT)
//                         u = dz - wn c (z - a r), dmu_k = u, dlv_k = 1/2 u (z - mu) + 1/2 wn
//                                                           PAeBwdT<true, true> (mode LATENT_IW)
//   weight gradients:     [in | 1]^T dout (ones row = bias gradient), prior -theta/s2 and
//                         AdaGrad (infalg.py:155-161) in the epilogue   PAeWgrad
//                         (or gradient ascent with momentum, AdaDelta, Adam: PAeWgradT<RULE>)
// The first layer's A operand is gathered on the fly through idx (no copy of Xtr[idx]).
// Every weight is updated only after the last kernel of the step that reads it, so the
// update is simultaneous in the Theano sense.
#pragma once
#include "tile_engine.hpp"

namespace vaeb {
namespace ae {

enum : int { ACT_TANH = 0, ACT_SIGMOID = 1, ACT_RELU = 2 };
enum : int { F_ACT = 0, F_LINEAR = 1, F_OUT_BIN = 2, F_OUT_CONT = 3, F_LATENT = 4, F_OUT_SE = 5 };
enum : int { B_DACT = 0, B_ZPRIOR = 1, B_LATENT = 2, B_LATENT_IW = 3 };
enum : int { NOISE_ZERO = 0, NOISE_HOST = 1, NOISE_PHILOX = 2 };   // eps of the F_LATENT epilogue
constexpr float kEpsLog = 1e-7f;   // logpdf.py:86
constexpr float kHalfLog2Pi = 0.91893853320467274178f;

struct Dbg { uint64_t* dbg; };

DEV float act_f(int act, float v) {
    if (act == ACT_TANH) return ftanh(v);
    if (act == ACT_SIGMOID) return sigmoidf(v);
    return fmaxf(v, 0.f);
}
DEV float dact_f(int act, float h) {   // in terms of the stored activation h
    if (act == ACT_TANH) return 1.f - h * h;
    if (act == ACT_SIGMOID) return h * (1.f - h);
    return h > 0.f ? 1.f : 0.f;
}

// element (r, k) of a row-major [rows x ld] matrix, 0 outside [0, rlim) x [0, klim)
DEV float el(rsrc_t b, int ld, int r, int k, int rlim, int klim) {
    return bld(b, (r < rlim && k < klim && r >= 0) ? (uint32_t)(r * ld + k) * 4u : kOOB);
}

// ---------------------------------------------------------------- forward layer
// F_OUT_SE (one head): per-(row, 16-column tile) partials of se = sum (Y - P)^2 in llpart, the
// delta 2 (Y - P) P (1 - P) in dA and P in out; Y with dA == nullptr: the partials only, as the
// other output modes.  The branch exists only in PAeFwdT<true> (the kernel arguments are the
// same), so PAeFwd's kernels are what they were without it.
//
// The two-mode latent prior (TM): a = mean1, c = 1 / width^2 and log(2 width), by value.  The
// three arguments and the branches that read them exist only in the TM instantiations of
// PAeFwdT and PAeBwdT (an empty base otherwise), so every other kernel and its arguments are what
// they were without them.  t = a (2 z - a) c / 2; softplus in its max(t, 0) + log(1 + e^-|t|)
// form (t reaches 1e3 at small widths: e^t is inf in float32) and r = sigmoid(t) from the same
// e^-|t|.
template <bool TM> struct AePriorArgs {};
template <> struct AePriorArgs<true> {
    float pa, pc, plog2s;
    DEV float t_of(float z) const { return 0.5f * pa * (2.f * z - pa) * pc; }
    // log p(z) + 1/2 log 2 pi
    DEV float logp(float z) const { return softplusf(t_of(z)) - plog2s - 0.5f * pc * z * z; }
    // -dlog p / dz = c (z - a r)
    DEV float pull(float z) const {
        const float t = t_of(z), e = fexp(-fabsf(t)), q = frcp(1.f + e);
        return pc * (z - pa * (t >= 0.f ? q : e * q));
    }
};

template <bool SE, bool TM = false>
struct PAeFwdT : AePriorArgs<TM> {
    Dbg a;
    int M, N, K;
    const float* in; int ldin; int in_rows; const int* idx;   // idx: gathered input rows
    const float *W, *W2, *b, *b2;                             // W [K x N] (W2: Wlogs2)
    int mode, act;
    float *out, *out2;                                        // activations / Xpr (+ ls2)
    const float* Y; const int* yidx; int ldy; int y_rows;     // observations (output layer)
    float *dA, *dA2;                                          // output deltas; Y with dA == nullptr: value
                                                              // only (llpart; no out / out2 / delta stores)
    float* llpart; int nct;                                   // [M][nct] log-lik partials
    // F_LATENT (W / W2 = Wzmu / Wzlv): out = mu, out2 = lv, zout = z, llpart = -KL partials.
    // eps: 0, eps_in[m][n] (host mode) or Philox keyed by c0 = erow[m] (the dataset row of a
    // training step) or erow0 + m (the row's index in an evaluation call's x), c1 = n.
    float* zout; int noise; const float* eps_in; const int* erow; uint32_t erow0;
    uint64_t seed; int64_t step; uint32_t domain;             // c2, c3 = philox_c23(step, domain)
    rsrc_t bin, bw, bw2, by;
    DEV void prepare() {
        bin = mkbuf(in, (int64_t)in_rows * ldin * 4);
        bw = mkbuf(W, (int64_t)K * N * 4);
        bw2 = mkbuf(W2 ? W2 : W, (int64_t)K * N * 4);
        by = mkbuf(Y ? Y : in, (int64_t)(Y ? y_rows : in_rows) * (Y ? ldy : ldin) * 4);
    }
    DEV int row_of(int m) const { return m < M ? (idx ? idx[m] : m) : -1; }
    DEV f32x4 a4(int m, int k) const {
        const int r = row_of(m);
        f32x4 v;
        v.x = el(bin, ldin, r, k + 0, in_rows, K);
        v.y = el(bin, ldin, r, k + 1, in_rows, K);
        v.z = el(bin, ldin, r, k + 2, in_rows, K);
        v.w = el(bin, ldin, r, k + 3, in_rows, K);
        return v;
    }
    DEV f32x4 b4(int n, int k, int w) const { return mc4(w ? bw2 : bw, N, n, k, N, K); }
    using Pre = NoPre;
    DEV Pre prefetch(int, int) const { return Pre{}; }
    template <int NB>
    DEV void epilogue(int m0, int n0, const f32x4 (&acc)[NB], const Pre&) const {
        const int lane = threadIdx.x & 63;
        const int n = n0 + (lane & 15);
        const bool nok = n < N;
        const float bb = nok ? b[n] : 0.f;
        const float bb2 = (nok && b2) ? b2[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * (lane >> 4) + r;
            const bool ok = nok && m < M;
            const float v = acc[0][r] + bb;
            if (mode == F_ACT || mode == F_LINEAR) {
                if (ok) out[(int64_t)m * N + n] = (mode == F_ACT) ? act_f(act, v) : v;
                continue;
            }
            if (mode == F_LATENT) {
                if constexpr (NB > 1) {
                    const float lv = acc[1][r] + bb2;
                    float e = 0.f;
                    if (noise == NOISE_HOST) e = ok ? eps_in[(int64_t)m * N + n] : 0.f;
                    else if (noise == NOISE_PHILOX)
                        e = philox_normal(seed, m < M ? (erow ? (uint32_t)erow[m] : erow0 + (uint32_t)m) : 0u,
                                          (uint32_t)n, philox_c23(step, domain));
                    const float sd = fexp(0.5f * lv);
                    if constexpr (TM) {   // the prior term at the sample z, the entropy analytic
                        const float z = (noise == NOISE_ZERO) ? v : v + sd * e;
                        if (ok) {
                            out[(int64_t)m * N + n] = v;
                            out2[(int64_t)m * N + n] = lv;
                            zout[(int64_t)m * N + n] = z;
                        }
                        const float s = sum16(ok ? 0.5f * (1.f + lv) + this->logp(z) : 0.f);
                        if ((lane & 15) == 0 && m < M) llpart[(int64_t)m * nct + n0 / 16] = s;
                        continue;
                    }
                    if (ok) {
                        out[(int64_t)m * N + n] = v;
                        out2[(int64_t)m * N + n] = lv;
                        zout[(int64_t)m * N + n] = (noise == NOISE_ZERO) ? v : v + sd * e;
                    }
                    const float s = sum16(ok ? 0.5f * (1.f + lv - v * v - sd * sd) : 0.f);
                    if ((lane & 15) == 0 && m < M) llpart[(int64_t)m * nct + n0 / 16] = s;
                }
                continue;
            }
            if (!Y) {   // predictions only (reconstruct / decode): Xpr (+ ls2)
                if (ok) out[(int64_t)m * N + n] = sigmoidf(v);
                if constexpr (NB > 1)
                    if (ok) out2[(int64_t)m * N + n] = acc[1][r] + bb2;
                continue;
            }
            const int yr = ok ? (yidx ? yidx[m] : m) : 0;
            const float y = ok ? Y[(int64_t)yr * ldy + n] : 0.f;
            if constexpr (SE) {
                if (mode == F_OUT_SE) {
                    const float P = sigmoidf(v), rr = y - P;
                    if (ok && dA) {
                        out[(int64_t)m * N + n] = P;
                        dA[(int64_t)m * N + n] = 2.f * rr * P * (1.f - P);
                    }
                    const float s = sum16(ok ? rr * rr : 0.f);
                    if ((lane & 15) == 0 && m < M) llpart[(int64_t)m * nct + n0 / 16] = s;
                    continue;
                }
            }
            float ll = 0.f;
            if (mode == F_OUT_BIN) {
                const float P = sigmoidf(v);
                ll = y * flog(P + kEpsLog) + (1.f - y) * flog(1.f - P + kEpsLog);
                if (dA) {
                    const float dP = y / (P + kEpsLog) - (1.f - y) / (1.f - P + kEpsLog);
                    if (ok) {
                        out[(int64_t)m * N + n] = P;
                        dA[(int64_t)m * N + n] = dP * P * (1.f - P);
                    }
                }
            } else {
                float ls2 = bb2;
                if constexpr (NB > 1) ls2 += acc[1][r];
                const float mu = sigmoidf(v);
                const float rr = y - mu, e = fexp(-ls2);
                ll = -kHalfLog2Pi - 0.5f * ls2 - 0.5f * rr * rr * e;
                if (ok && dA) {
                    out[(int64_t)m * N + n] = mu;
                    out2[(int64_t)m * N + n] = ls2;
                    dA[(int64_t)m * N + n] = rr * e * mu * (1.f - mu);
                    dA2[(int64_t)m * N + n] = -0.5f + 0.5f * rr * rr * e;
                }
            }
            const float s = sum16(ok ? ll : 0.f);
            if ((lane & 15) == 0 && m < M) llpart[(int64_t)m * nct + n0 / 16] = s;
        }
    }
};

using PAeFwd = PAeFwdT<false>;
using PAeFwdSe = PAeFwdT<true>;
using PAeFwdTm = PAeFwdT<false, true>;   // F_LATENT under the two-mode prior (2 heads)

// ---------------------------------------------------------------- backward (data) layer
// din[M x N] = [dout | dout2] [W | W2]^T  (K = K1 or 2 K1), then * f'(h) or - h (Z prior).
// B_LATENT (the decoder's first layer, N = Dz): dz = dout W^T, h / h2 / h3 = mu / lv / z,
// din = dmu = dz - mu, din2 = dlv = 1/2 dz (z - mu) + 1/2 (1 - e^lv).
// B_LATENT_IW (training on the importance-weighted bound, ae_iwae.hpp): M = K * Mp stacked rows,
// dout already carries the normalised weight wn of its row; stacked row g reads mu / lv at row
// g mod Mp and z / wn at g:  u = dz - wn z,  din = dmu_k = u,  din2 = dlv_k = 1/2 u (z - mu) + 1/2 wn
// (no analytic KL: the latent term of log w is differentiated as it stands).  The branch and its
// two arguments exist only in PAeBwdT<true>, so PAeBwd's kernels and kernel arguments are what
// they were without it.
// Two-mode prior (TM, AePriorArgs above): B_LATENT g = dz - c (z - a r), din = g,
// din2 = 1/2 g (z - mu) + 1/2 (lv is not read); B_LATENT_IW u = dz - wn c (z - a r).
template <bool IW> struct AeBwdIwArgs {};
template <> struct AeBwdIwArgs<true> { const float* wt; int Mp; };   // wn [M], rows per sample plane
template <bool IW, bool TM = false>
struct PAeBwdT : AeBwdIwArgs<IW>, AePriorArgs<TM> {
    Dbg a;
    int M, N, K;
    const float *dout, *dout2; int K1;
    const float *W, *W2;             // [N x K1] each (row n = this layer's input unit)
    const float* h; int mode, act;   // h [M x N]: activation (DACT) or Z (ZPRIOR)
    float* din;
    const float *h2, *h3; float* din2;   // B_LATENT / B_LATENT_IW only
    rsrc_t bd, bd2, bw, bw2;
    DEV void prepare() {
        bd = mkbuf(dout, (int64_t)M * K1 * 4);
        bd2 = mkbuf(dout2 ? dout2 : dout, (int64_t)M * K1 * 4);
        bw = mkbuf(W, (int64_t)N * K1 * 4);
        bw2 = mkbuf(W2 ? W2 : W, (int64_t)N * K1 * 4);
    }
    DEV float src(rsrc_t b1, rsrc_t b2, int r, int k, int rl) const {
        return k < K1 ? el(b1, K1, r, k, rl, K1) : el(b2, K1, r, k - K1, rl, K1);
    }
    DEV f32x4 a4(int m, int k) const {
        f32x4 v;
        v.x = src(bd, bd2, m, k + 0, M);
        v.y = src(bd, bd2, m, k + 1, M);
        v.z = src(bd, bd2, m, k + 2, M);
        v.w = src(bd, bd2, m, k + 3, M);
        if (k + 0 >= K) v.x = 0.f;
        if (k + 1 >= K) v.y = 0.f;
        if (k + 2 >= K) v.z = 0.f;
        if (k + 3 >= K) v.w = 0.f;
        return v;
    }
    DEV f32x4 b4(int n, int k, int) const {
        f32x4 v;
        v.x = src(bw, bw2, n, k + 0, N);
        v.y = src(bw, bw2, n, k + 1, N);
        v.z = src(bw, bw2, n, k + 2, N);
        v.w = src(bw, bw2, n, k + 3, N);
        return v;
    }
    using Pre = NoPre;
    DEV Pre prefetch(int, int) const { return Pre{}; }
    template <int NB>
    DEV void epilogue(int m0, int n0, const f32x4 (&acc)[NB], const Pre&) const {
        const int lane = threadIdx.x & 63;
        const int n = n0 + (lane & 15);
        if (n >= N) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * (lane >> 4) + r;
            if (m >= M) continue;
            if constexpr (IW) {
                if (mode == B_LATENT_IW) {
                    const int64_t o = (int64_t)m * N + n, om = (int64_t)(m % this->Mp) * N + n;
                    const float w = this->wt[m], z = h3[o], mu = h[om];
                    float u;
                    if constexpr (TM) u = acc[0][r] - w * this->pull(z);
                    else u = acc[0][r] - w * z;
                    din[o] = u;
                    din2[o] = 0.5f * u * (z - mu) + 0.5f * w;
                    continue;
                }
            }
            const float hv = h[(int64_t)m * N + n];
            if constexpr (TM) {
                if (mode == B_LATENT) {
                    const float z = h3[(int64_t)m * N + n];
                    const float g = acc[0][r] - this->pull(z);
                    din[(int64_t)m * N + n] = g;
                    din2[(int64_t)m * N + n] = 0.5f * g * (z - hv) + 0.5f;
                    continue;
                }
            }
            if (mode == B_LATENT) {
                const float dz = acc[0][r], lv = h2[(int64_t)m * N + n], z = h3[(int64_t)m * N + n];
                din[(int64_t)m * N + n] = dz - hv;
                din2[(int64_t)m * N + n] = 0.5f * dz * (z - hv) + 0.5f * (1.f - fexp(lv));
                continue;
            }
            din[(int64_t)m * N + n] = (mode == B_DACT) ? acc[0][r] * dact_f(act, hv) : acc[0][r] - hv;
        }
    }
};
using PAeBwd = PAeBwdT<false>;

// ---------------------------------------------------------------- weight gradient + update rule
// C[Kin + 1 x N] = [in | 1]^T dout over the M batch rows (row Kin = the bias gradient),
// g = C - theta / s2 (mlp.py:87-91 prior), then the context's rule (include/vaeb_hip.h enum
// vaeb_ae_rule), every rule ascending.  accum is slot 0 of the optimiser state, state1 slot 1,
// both indexed as theta; element (m, n) of theta belongs to one lane, which reads and writes its
// theta and state with plain loads and stores:
//   RULE_ADAGRAD   (infalg.py:155-161)  acc += g^2, theta += eta g / (sqrt(acc) + 1e-6)
//   RULE_SGA       (infalg.py:44-74 + momentum)  v' = mu v + g, theta += eta v'
//                  (mu = 0: slot 0 holds g, stored as computed -- the engine's gradient read-out)
//   RULE_ADADELTA  (infalg.py:88-106)   g_ac' = rho g_ac + (1 - rho) g^2,
//                  dx = sqrt(dx_ac + eps) g / sqrt(g_ac' + eps), theta += eta dx,
//                  dx_ac' = rho dx_ac + (1 - rho) dx^2          (slot 0 g_ac, slot 1 dx_ac)
//   RULE_ADAM      m' = b1 m + (1 - b1) g, v' = b2 v + (1 - b2) g^2,
//                  theta += eta (m' / bc1) / (sqrt(v' / bc2) + eps)   (slot 0 m, slot 1 v;
//                  bc_i = 1 - b_i^t by value: the host forms them per step in double)
// A rule's extra arguments and its branch exist only in its own instantiation (an empty base for
// AdaGrad), so PAeWgrad's kernel and kernel arguments are what they were without the others.
enum : int { RULE_ADAGRAD = 0, RULE_SGA = 1, RULE_ADADELTA = 2, RULE_ADAM = 3 };
template <int RULE> struct AeRuleArgs {};
template <> struct AeRuleArgs<RULE_SGA> { float mu; };
template <> struct AeRuleArgs<RULE_ADADELTA> { float* state1; float rho, eps; };
template <> struct AeRuleArgs<RULE_ADAM> { float* state1; float b1, b2, eps, bc1, bc2; };

// Weight dropout (MASK, the classifier's dropout contexts; clf_softmax.hpp): the forward and the
// data backward ran on theta~ = theta * m, so the gradient with respect to theta is m * C; the byte
// mask m (indexed as theta) selects C or 0 before the prior term, and the rule updates the real
// theta: a dropped element sees g = -theta / s2.  The argument and the select exist only in the
// MASK instantiations (an empty base otherwise), so every other kernel is what it was.
template <bool MASK> struct AeMaskArgs {};
template <> struct AeMaskArgs<true> { const uint8_t* mask; };

template <int RULE, bool MASK = false>
struct PAeWgradT : AeRuleArgs<RULE>, AeMaskArgs<MASK> {
    Dbg a;
    int M, N, K;                     // M = Kin + 1, N = out width, K = batch rows
    const float* in; int ldin; int in_rows; const int* idx; int Kin;
    const float* dout;
    float *theta, *accum; int64_t offW, offb;
    float eta, inv_s2;
    rsrc_t bin, bd;
    DEV void prepare() {
        bin = mkbuf(in, (int64_t)in_rows * ldin * 4);
        bd = mkbuf(dout, (int64_t)K * N * 4);
    }
    DEV float ina(int m, int k) const {
        if (k >= K) return 0.f;
        if (m == Kin) return 1.f;
        const int r = idx ? idx[k] : k;
        return el(bin, ldin, r, m, in_rows, Kin);
    }
    DEV f32x4 a4(int m, int k) const {
        f32x4 v;
        v.x = ina(m, k + 0);
        v.y = ina(m, k + 1);
        v.z = ina(m, k + 2);
        v.w = ina(m, k + 3);
        return v;
    }
    DEV f32x4 b4(int n, int k, int) const { return mc4(bd, N, n, k, N, K); }
    using Pre = NoPre;
    DEV Pre prefetch(int, int) const { return Pre{}; }
    template <int NB>
    DEV void epilogue(int m0, int n0, const f32x4 (&acc)[NB], const Pre&) const {
        const int lane = threadIdx.x & 63;
        const int n = n0 + (lane & 15);
        if (n >= N) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * (lane >> 4) + r;
            if (m > Kin) continue;
            const int64_t i = (m == Kin) ? offb + n : offW + (int64_t)m * N + n;
            const float th = theta[i];
            float c = acc[0][r];
            if constexpr (MASK) c = this->mask[i] ? c : 0.f;
            const float g = c - th * inv_s2;
            if constexpr (RULE == RULE_SGA) {
                const float v = this->mu * accum[i] + g;
                accum[i] = v;
                theta[i] = th + eta * v;
            } else if constexpr (RULE == RULE_ADADELTA) {
                const float dxa = this->state1[i];
                const float ga = this->rho * accum[i] + (1.f - this->rho) * (g * g);
                const float dx = sqrtf(dxa + this->eps) * g / sqrtf(ga + this->eps);
                accum[i] = ga;
                this->state1[i] = this->rho * dxa + (1.f - this->rho) * (dx * dx);
                theta[i] = th + eta * dx;
            } else if constexpr (RULE == RULE_ADAM) {
                const float m1 = this->b1 * accum[i] + (1.f - this->b1) * g;
                const float v1 = this->b2 * this->state1[i] + (1.f - this->b2) * (g * g);
                accum[i] = m1;
                this->state1[i] = v1;
                theta[i] = th + eta * (m1 / this->bc1) / (sqrtf(v1 / this->bc2) + this->eps);
            } else {
                const float ac = accum[i] + g * g;
                accum[i] = ac;
                theta[i] = th + eta * g / (sqrtf(ac) + 1e-6f);
            }
        }
    }
};
using PAeWgrad = PAeWgradT<RULE_ADAGRAD>;

// Log-likelihood of the step: fixed-order fp64 sum of the [M][nct] partials -> out[slot]
// (= loglik / M, the value train() returns, ae.py:86).
__global__ __launch_bounds__(256) void ae_loglik_kernel(const float* part, int64_t n, int M, float* out, int slot) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += part[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[slot] = (float)(sh[0] / (double)M);
}

// vaeb_ae_sq_error: rows[m] = the row's nct squared-error partials added in ascending tile order
// (float, one thread per row: the value depends on the row alone, not on the chunk it falls in).
__global__ __launch_bounds__(256) void ae_row_sum_kernel(const float* part, int M, int nct, float* rows) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float s = 0.f;
    for (int t = 0; t < nct; ++t) s += part[(int64_t)m * nct + t];
    rows[m] = s;
}

// Gaussian latent: the step's value (loglik - KL) / M from the log-lik and the -KL partials,
// each summed in a fixed order in fp64 -> out[slot]; sum_out (vaeb_ae_elbo): the sum itself.
__global__ __launch_bounds__(256) void ae_elbo_kernel(const float* llpart, int64_t nll, const float* klpart, int64_t nkl,
                                                      int M, float* out, int slot, double* sum_out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < nll; i += 256) s += llpart[i];
    for (int64_t i = threadIdx.x; i < nkl; i += 256) s += klpart[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (out) out[slot] = (float)(sh[0] / (double)M);
        if (sum_out) *sum_out = sh[0];
    }
}

}  // namespace ae
}  // namespace vaeb
