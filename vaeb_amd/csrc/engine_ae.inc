// engine_ae.inc -- the layer-stack engine (include/vaeb_hip.h vaeb_ae_*): the autoencoders and
// deep VAEs on the fp32 tile engine's kernels (ae_mlp.hpp, ae_iwae.hpp).  Included by
// vaeb_hip.hip after stack_core.inc: vaeb_ae is a StackCore, and the launches of the plain forward
// layers, of every data gradient and of every update, the update rule's calls, the training
// driver, the chunk loop (ae_chunks: core_chunks on xin) and the chunk sum are the core's.
// Each call and the helper sequence it runs:
//   vaeb_ae_train(_many)  core_train_many, per batch ae_step: ae_encode | ae_decode_hidden | ae_output(TRAIN) | the value
//                         (iw_samples >= 2: ae_iw_forward instead), then ae_bwd_decoder | ae_bwd_encoder;
//                         on a corrupting context ae_corrupt_rows first: ae_encode and ae_bwd_encoder read
//                         its xt, everything else the clean rows
//   vaeb_ae_corrupt       chunks of max_batch: ae_corrupt_rows, xt to the host
//   vaeb_ae_reconstruct   ae_chunks: ae_encode (zero noise) | ae_decode_hidden | ae_output(PREDICT)
//   vaeb_ae_encode        ae_chunks: ae_encode (zero noise)
//   vaeb_ae_decode        ae_chunks: ae_decode_hidden on the caller's z | ae_output(PREDICT)
//   vaeb_ae_sq_error      ae_chunks: ae_encode (zero noise) | ae_decode_hidden | ae_output(SQ) |
//                         ae_row_sum_kernel | core_sum_to_host
//   vaeb_ae_encode_dist   ae_chunks: ae_encode (evaluation noise when z is wanted)
//   vaeb_ae_elbo          ae_chunks: ae_encode (evaluation noise) | ae_decode_hidden | ae_output(TRAIN) |
//                         ae_elbo_kernel | core_sum_to_host
//   vaeb_ae_marginal_ll   ae_chunks: ae_encode (zero noise), per pass of sample planes ae_iw_sample_kernel |
//                         ae_decode_hidden | ae_output(VALUE) | iw_lse_kernel, then core_sum_to_host
//   vaeb_ae_encode_bits   ae_chunks: ae_encode (zero noise) | ae_pack_bits_kernel
//   vaeb_ae_decode_bits   ae_chunks: ae_unpack_bits_kernel | ae_decode_hidden | ae_output(PREDICT)
//   vaeb_ae_set_optimizer core_set_optimizer: the rule and hyper-parameters core_wgrad launches with
//                         (PAeWgradT<RULE>); another rule: both state slots and the optimiser step
//                         counter zeroed on the stream
// A context of the two-mode latent prior (c.prior, ae_two_mode) runs the same sequences with the TM
// instantiations of the latent forward, the decoder's first-layer backward and the sample kernel;
// every other context launches what it launched before.
// vaeb_ae_create lays theta out (an AeLayer per layer and head); device memory is the context's:
// StackCore::mem (dev_owner.hpp) registers every buffer where it is allocated, core_close releases it.

// A layer of one or two heads on the same input (the latent: Wz, or Wzmu and Wzlv; the output:
// Wout, or Wmu and Wlogs2) with the deltas of the heads' pre-activations.
struct AeHeads { int n; AeLayer l[2]; float* d[2]; };

struct vaeb_ae : StackCore {
    vaeb_ae_config c{};
    AeLayer enc[VAEB_AE_MAX_LAYERS] = {}, dec[VAEB_AE_MAX_LAYERS] = {};   // Dobs -> Denc..., Dz -> Ddec...
    AeHeads lat{}, out{};             // d: dZ, or dmu and dlv (Gaussian latent); dA (and dA2, cont)
    float* data = nullptr;
    int64_t nrows = 0;
    // activations / deltas per layer (H[0], G[0] unused)
    float *H[VAEB_AE_MAX_LAYERS + 1] = {}, *G[VAEB_AE_MAX_LAYERS + 1] = {};
    float *dH[VAEB_AE_MAX_LAYERS + 1] = {}, *dG[VAEB_AE_MAX_LAYERS + 1] = {};
    float *Z = nullptr, *dZ = nullptr, *Xpr = nullptr, *ls2 = nullptr, *dA = nullptr, *dA2 = nullptr;
    float *ll = nullptr, *xin = nullptr;
    // Gaussian latent (c.latent == VAEB_AE_LATENT_GAUSS): a->Z holds z
    float *mu = nullptr, *lv = nullptr, *dmu = nullptr, *dlv = nullptr, *kl = nullptr;
    // esum (the core's): vaeb_ae_elbo / vaeb_ae_marginal_ll / vaeb_ae_sq_error, one chunk's sum
    float* sq_rows = nullptr;         // vaeb_ae_sq_error: a chunk's row values [max_batch] (first use)
    // vaeb_ae_marginal_ll scratch (allocated on first use): latent terms [max_batch], running
    // (max, sum) [2 max_batch], row values [max_batch]; the observation row of each stacked row
    float* iw = nullptr;
    int* iw_yrow = nullptr;
    // training on the importance-weighted bound (c.iw_samples >= 2; allocated at create):
    // normalised weights [max_batch], row values [max_batch], log w / exp scratch [max_batch]
    float *iw_wt = nullptr, *iw_val = nullptr;
    double* iw_lw = nullptr;
    int eps_mode = VAEB_EPS_PHILOX;
    uint64_t seed = 0;
    int64_t step = 0;                 // Philox step counter
    float* eps_in = nullptr;          // pushed host eps [eps_rows x Dz]
    int64_t eps_rows = 0, eps_cap = 0;
    // input corruption (c.corruption != VAEB_AE_CORRUPT_NONE; ae_corrupt.hpp): the corrupted rows
    // xt [max_batch x Dobs] (allocated at create), the level, and a noise mode, seed and pushed
    // draws [cor_rows x Dobs] of its own; the step counter is the one above
    float* xc = nullptr;
    float cor_level = 0.f;
    int cor_mode = VAEB_EPS_PHILOX;
    uint64_t cor_seed = 0;
    float* cor_in = nullptr;
    int64_t cor_rows = 0, cor_cap = 0;
    // the two-mode latent prior (c.prior == VAEB_AE_PRIOR_TWO_MODE): mean1 and width, launch
    // arguments as the level above; a chunk's code words [max_batch x ceil(Dz / 32)] (first use)
    float pr_mean1 = 1.f, pr_width = 0.25f;
    uint32_t* code_w = nullptr;
};

namespace {

bool ae_gauss(const vaeb_ae* a) { return a->c.latent == VAEB_AE_LATENT_GAUSS; }
bool ae_act_latent(const vaeb_ae* a) { return a->c.latent == VAEB_AE_LATENT_ACT; }
bool ae_iw(const vaeb_ae* a) { return a->c.iw_samples >= 2; }
bool ae_corrupting(const vaeb_ae* a) { return a->c.corruption != VAEB_AE_CORRUPT_NONE; }
bool ae_two_mode(const vaeb_ae* a) { return a->c.prior == VAEB_AE_PRIOR_TWO_MODE; }

// The prior's launch arguments a, c = 1 / s^2 and log(2 s) into a TM parameter block (nothing
// into any other: the overload is chosen by the block's base).
void ae_put_prior(const vaeb_ae*, ae::AePriorArgs<false>&) {}
void ae_put_prior(const vaeb_ae* a, ae::AePriorArgs<true>& q) {
    const double s = a->pr_width;
    q.pa = a->pr_mean1; q.pc = (float)(1.0 / (s * s)); q.plog2s = (float)std::log(2.0 * s);
}

// vaeb_ae_marginal_ll's and the importance-weighted step's scratch, sized by max_batch
int ae_iw_scratch(vaeb_ae* a) {
    const int64_t B = a->c.max_batch;
    if (int rc = a->mem.lazy(&a->iw, 4 * B)) return rc;
    return a->mem.lazy(&a->iw_yrow, B);
}

// ------------------------------------------------------------------ forward
// eps of one latent forward (ae::PAeFwd F_LATENT): zero (the deterministic predictions), or the
// noise of rows [r0, r0 + ...) of a call in the context's eps mode: rows of the pushed host eps, or
// Philox at the step counter, for training (domain 0, keyed by the dataset rows `rows`) or
// evaluation (domain 1, stream 0, keyed by r0 + m).
enum AeEps { AE_EPS_ZERO, AE_EPS_TRAIN, AE_EPS_EVAL };
struct AeNoise { AeEps kind; const int* rows; int64_t r0; };

int ae_host_eps_ready(const vaeb_ae* a, int64_t rows) {
    if (a->eps_mode == VAEB_EPS_HOST && a->eps_rows != rows)
        return fail(VAEB_ERR_STATE, "host eps mode: pushed %lld rows, the call needs %lld (call vaeb_ae_push_eps)",
                    (long long)a->eps_rows, (long long)rows);
    return 0;
}

int ae_host_corruption_ready(const vaeb_ae* a, int64_t rows) {
    if (ae_corrupting(a) && a->cor_mode == VAEB_EPS_HOST && a->cor_rows != rows)
        return fail(VAEB_ERR_STATE, "host corruption noise: pushed %lld rows, the call needs %lld (call vaeb_ae_push_corruption)",
                    (long long)a->cor_rows, (long long)rows);
    return 0;
}

// xt = the M dataset rows idx, corrupted at the context's level and step, into a->xc.  lb: the
// rows' offset in the call's idx list (host mode: the pushed draws of list position lb + m).
int ae_corrupt_rows(vaeb_ae* a, const int* idx, int M, int64_t lb) {
    ae::AeCorruptArgs q{};
    q.X = a->data; q.x_rows = (int)a->nrows; q.idx = idx; q.M = M; q.D = a->c.Dobs;
    q.kind = a->c.corruption; q.level = a->cor_level;
    q.rin = a->cor_mode == VAEB_EPS_HOST ? a->cor_in + lb * a->c.Dobs : nullptr;
    q.seed = a->cor_seed; q.step = a->step; q.out = a->xc;
    hipLaunchKernelGGL(ae::ae_corrupt_kernel, dim3(cdiv(M * a->c.Dobs, 256)), dim3(256), 0, a->s, q);
    CHECK_LAUNCH();
    return 0;
}

// out = f(in W + b) (ae::F_ACT) or in W + b (ae::F_LINEAR) under theta
int ae_fwd_layer(vaeb_ae* a, const AeLayer& l, const AeRows& in, int M, int mode, float* out) {
    return core_fwd_layer(a, a->theta, l, in, M, mode, out);
}

// Encoder and latent for the M rows of x: H[], then Z, or with a Gaussian latent mu, lv, the -KL
// partials kl and Z = mu + exp(lv / 2) eps, eps from nz.
int ae_encode(vaeb_ae* a, const AeRows& x, int M, const AeNoise& nz) {
    const int ne = a->c.n_enc;
    for (int i = 0; i < ne; ++i)
        if (int rc = ae_fwd_layer(a, a->enc[i], i == 0 ? x : AeRows{a->H[i], M}, M, ae::F_ACT, a->H[i + 1])) return rc;
    const AeRows h{a->H[ne], M};
    if (!ae_gauss(a))   // Z = H Wz + bz, or f of it (the activated latent)
        return ae_fwd_layer(a, a->lat.l[0], h, M, ae_act_latent(a) ? ae::F_ACT : ae::F_LINEAR, a->Z);
    auto latent = [&](auto p) {   // two-mode prior: kl holds the latent_row partials at z
        p = ae_fwd_args<decltype(p)>(a->theta, a->lat.l[0], h, M);
        p.W2 = a->theta + a->lat.l[1].oW; p.b2 = a->theta + a->lat.l[1].ob;
        p.mode = ae::F_LATENT; p.out = a->mu; p.out2 = a->lv; p.zout = a->Z;
        p.llpart = a->kl; p.nct = cdiv(a->c.Dz, 16);
        p.seed = a->seed;
        if (nz.kind != AE_EPS_ZERO && a->eps_mode == VAEB_EPS_HOST) {
            p.noise = ae::NOISE_HOST; p.eps_in = a->eps_in + nz.r0 * a->c.Dz;
        } else if (nz.kind != AE_EPS_ZERO) {
            p.noise = ae::NOISE_PHILOX; p.erow = nz.rows; p.erow0 = (uint32_t)nz.r0;
            p.step = a->step; p.domain = nz.kind == AE_EPS_EVAL ? 1u : 0u;
        }
        ae_put_prior(a, p);
        launch_bigk<2>(a->s, p);
    };
    if (ae_two_mode(a)) latent(ae::PAeFwdTm{});
    else latent(ae::PAeFwd{});
    CHECK_LAUNCH();
    return 0;
}

// The decoder's hidden layers for M rows of z (a->Z or a caller's): G[].
int ae_decode_hidden(vaeb_ae* a, const float* z, int M) {
    for (int i = 0; i < a->c.n_dec; ++i)
        if (int rc = ae_fwd_layer(a, a->dec[i], AeRows{i == 0 ? z : a->G[i], M}, M, ae::F_ACT, a->G[i + 1])) return rc;
    return 0;
}

// What the output layer leaves, for M rows of the last decoder activation:
enum AeOut {
    AE_OUT_PREDICT,   // the predictions Xpr (+ ls2); no observations
    AE_OUT_VALUE,     // the per-(row, 16-column tile) partials ll of the context's output value, nothing else
    AE_OUT_TRAIN,     // the partials, the predictions and the deltas dA (+ dA2)
    AE_OUT_SQ         // the partials of the mean head's squared error, whatever the context's otype
};

// y: the observation rows (all but AE_OUT_PREDICT).  The kernel: F_OUT_SE (PAeFwdSe, squared error:
// its own instantiation; the mean head l[0] alone) for AE_OUT_SQ and for the observed forms of a
// squared-error context, else by otype F_OUT_CONT (both heads) or F_OUT_BIN (binary, and the
// predictions of a squared-error context).  A kernel given Y and no dA leaves the partials only.
int ae_output(vaeb_ae* a, int M, AeOut what, const AeRows& y = AeRows{}) {
    const vaeb_ae_config& g = a->c;
    const bool obs = what != AE_OUT_PREDICT, deltas = what == AE_OUT_PREDICT || what == AE_OUT_TRAIN;
    const bool se = what == AE_OUT_SQ || (obs && g.otype == VAEB_AE_SE), cont = g.otype == VAEB_AE_CONT;
    auto args = [&](auto p, int mode) {
        p = ae_fwd_args<decltype(p)>(a->theta, a->out.l[0], AeRows{a->G[g.n_dec], M}, M);
        p.out = a->Xpr;
        if (obs) { p.Y = y.p; p.yidx = y.idx; p.ldy = g.Dobs; p.y_rows = y.rows; }
        p.dA = deltas ? a->dA : nullptr; p.llpart = a->ll; p.nct = cdiv(g.Dobs, 16);
        p.mode = mode;
        return p;
    };
    if (se) {
        launch_bigk<1>(a->s, args(ae::PAeFwdSe{}, ae::F_OUT_SE));
    } else if (!cont) {
        launch_bigk<1>(a->s, args(ae::PAeFwd{}, ae::F_OUT_BIN));
    } else {
        ae::PAeFwd p = args(ae::PAeFwd{}, ae::F_OUT_CONT);
        p.W2 = a->theta + a->out.l[1].oW; p.b2 = a->theta + a->out.l[1].ob; p.out2 = a->ls2;
        p.dA2 = deltas ? a->dA2 : nullptr;
        launch_bigk<2>(a->s, p);
    }
    CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ backward
// Backward through one layer of nh (1 or 2) heads l[] with the pre-activation deltas d[] on the
// input `in` over M rows (core_bwd_layer: the data gradient, then mode, into din with the old
// theta; din == nullptr: none; then each head's update with the prior's 1 / s2).  The latent modes
// read mu, lv and z and leave dmu and dlv; IW: the sample weights; TM: the prior's arguments.
template <bool IW = false, bool TM = false>
int ae_bwd_layer(vaeb_ae* a, const AeLayer* l, float* const* d, int nh, const AeRows& in, int M, int mode, float* din) {
    auto fill = [a, mode, M](ae::PAeBwdT<IW, TM>& p) {
        if (mode == ae::B_LATENT || mode == ae::B_LATENT_IW) {
            p.h = a->mu; p.h2 = a->lv; p.h3 = a->Z; p.din = a->dmu; p.din2 = a->dlv;
        }
        if constexpr (IW) { p.wt = a->iw_wt; p.Mp = M / a->c.iw_samples; }
        ae_put_prior(a, p);
    };
    return core_bwd_layer<ae::PAeBwdT<IW, TM>>(a, a->theta, l, d, nh, in, M, mode, din, 1.0f / a->c.s2, nullptr, fill);
}

// Output layer and decoder (top down) over R rows; dG[i+1] is the pre-activation delta of layer i.
// mode0 is the first decoder layer's: B_ZPRIOR (dZ = dz - Z), B_DACT (the activated latent: times
// f'(Z), no - Z), B_LATENT (dmu, dlv) or B_LATENT_IW (dmu_k, dlv_k per stacked row); the latter two
// in their TM instantiations on a context of the two-mode prior.
int ae_bwd_decoder(vaeb_ae* a, int R, int mode0) {
    const int nd = a->c.n_dec, act = ae::B_DACT;
    if (int rc = ae_bwd_layer(a, a->out.l, a->out.d, a->out.n, AeRows{a->G[nd], R}, R, act, a->dG[nd])) return rc;
    for (int i = nd - 1; i > 0; --i)
        if (int rc = ae_bwd_layer(a, &a->dec[i], &a->dG[i + 1], 1, AeRows{a->G[i], R}, R, act, a->dG[i])) return rc;
    const AeRows z{a->Z, R};
    if (ae_two_mode(a))
        return mode0 == ae::B_LATENT_IW ? ae_bwd_layer<true, true>(a, a->dec, &a->dG[1], 1, z, R, mode0, a->dZ)
                                        : ae_bwd_layer<false, true>(a, a->dec, &a->dG[1], 1, z, R, mode0, a->dZ);
    return mode0 == ae::B_LATENT_IW ? ae_bwd_layer<true>(a, a->dec, &a->dG[1], 1, z, R, mode0, a->dZ)
                                    : ae_bwd_layer(a, a->dec, &a->dG[1], 1, z, R, mode0, a->dZ);
}

// The latent layer Z = H Wz + bz (dZ: its pre-activation delta on the activated latent), or the
// two heads [mu | lv] = H [Wzmu | Wzlv] + [bzmu | bzlv], then the encoder (top down) over the M
// rows of x.
int ae_bwd_encoder(vaeb_ae* a, const AeRows& x, int M) {
    const int ne = a->c.n_enc, act = ae::B_DACT;
    if (int rc = ae_bwd_layer(a, a->lat.l, a->lat.d, a->lat.n, AeRows{a->H[ne], M}, M, act, a->dH[ne])) return rc;
    for (int i = ne - 1; i > 0; --i)
        if (int rc = ae_bwd_layer(a, &a->enc[i], &a->dH[i + 1], 1, AeRows{a->H[i], M}, M, act, a->dH[i])) return rc;
    return ae_bwd_layer(a, a->enc, &a->dH[1], 1, x, M, act, nullptr);
}

// z, the latent terms and the gather list of `rows` stacked rows (ae_iwae.hpp), under the context's prior.
int ae_iw_sample(vaeb_ae* a, const ae::AeIwArgs& q, int rows) {
    if (ae_two_mode(a)) {
        ae::AePriorArgs<true> pr{};
        ae_put_prior(a, pr);
        hipLaunchKernelGGL(ae::ae_iw_sample_tm_kernel, dim3(cdiv(rows, 16)), dim3(256), 0, a->s, q, pr);
    } else {
        hipLaunchKernelGGL(ae::ae_iw_sample_kernel, dim3(cdiv(rows, 16)), dim3(256), 0, a->s, q);
    }
    CHECK_LAUNCH();
    return 0;
}

// The forward of a step on the K-sample importance-weighted bound (c.iw_samples = K >= 2,
// ae_iwae.hpp): the encoder once on the M rows, the decoder on the K * M stacked rows
// (g = k * M + m) with the output deltas scaled by the normalised weights.  L_K / M -> outs[slot].
// lb: the step's offset in the call's idx list of n rows (host eps: sample k of list position i
// at row k * n + i).  xe: the encoder's input rows (x, or its corrupted copy); x keeps the row
// identity (the Philox c0) and the observations.
int ae_iw_forward(vaeb_ae* a, const AeRows& xe, const AeRows& x, int M, int slot, int64_t lb, int64_t n) {
    const vaeb_ae_config& g = a->c;
    const int D = g.Dobs, K = g.iw_samples, KM = K * M;
    if (int rc = ae_encode(a, xe, M, AeNoise{})) return rc;   // mu, lv
    ae::AeIwArgs q{};
    q.Dz = g.Dz; q.R = M; q.S = K; q.k0 = 0; q.row0 = lb; q.n = n;
    q.eps_mode = a->eps_mode == VAEB_EPS_HOST ? 1 : 0;
    q.seed = a->seed; q.step = a->step; q.eps_in = a->eps_in;
    q.mu = a->mu; q.lv = a->lv; q.z = a->Z; q.lat = a->iw; q.yrow = a->iw_yrow; q.idx = x.idx;
    if (int rc = ae_iw_sample(a, q, KM)) return rc;
    if (int rc = ae_decode_hidden(a, a->Z, KM)) return rc;
    if (int rc = ae_output(a, KM, AE_OUT_TRAIN, AeRows{x.p, x.rows, a->iw_yrow})) return rc;
    ae::AeIwWeightArgs w{};
    w.M = M; w.K = K; w.D = D; w.nct = cdiv(D, 16); w.logK = std::log((double)K);
    w.llpart = a->ll; w.lat = a->iw; w.lw = a->iw_lw; w.wt = a->iw_wt; w.rowval = a->iw_val;
    w.dA = a->dA; w.dA2 = g.otype == VAEB_AE_CONT ? a->dA2 : nullptr;
    hipLaunchKernelGGL(ae::ae_iw_weight_kernel, dim3(M), dim3(256), 0, a->s, w);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(ae::ae_loglik_kernel, dim3(1), dim3(256), 0, a->s, a->iw_val, (int64_t)M, M, a->outs, slot);
    CHECK_LAUNCH();
    return 0;
}

// train(idx) on the M dataset rows idx (the slice at offset lb of the call's list of n rows):
// forward + value, then the backward.  loglik / M -> outs[slot]; Gaussian latent: (loglik - KL) / M,
// eps drawn at the step counter, which then advances (the one place; point contexts have none).
// A corrupting context: the encoder's input rows xe are the corrupted copy a->xc of x (drawn at
// the same step counter, which advances once whatever the latent), read by the first layer's
// forward and weight gradient; the observations, the latent draw's c0 and the host-eps offsets
// stay those of x and idx.  Without corruption xe is x: the launches are what they were.
// Squared-error output: the partials are se, so outs[slot] = se / M (positive) while the deltas
// are those of -se.  iw_samples >= 2: ae_iw_forward, the decoder's backward on the K * M stacked
// rows, the K planes of dmu / dlv summed, then the encoder's backward on M rows as ever.
int ae_step(vaeb_ae* a, const int* idx, int M, int slot, int64_t lb, int64_t n) {
    const vaeb_ae_config& g = a->c;
    const bool gauss = ae_gauss(a), iw = ae_iw(a);
    const AeRows x{a->data, (int)a->nrows, idx};
    AeRows xe = x;
    if (ae_corrupting(a)) {
        if (int rc = ae_corrupt_rows(a, idx, M, lb)) return rc;
        xe = AeRows{a->xc, M, nullptr};
    }
    const int R = iw ? g.iw_samples * M : M;
    if (iw) {
        if (int rc = ae_iw_forward(a, xe, x, M, slot, lb, n)) return rc;
    } else {
        if (int rc = ae_encode(a, xe, M, AeNoise{AE_EPS_TRAIN, idx, lb})) return rc;
        if (int rc = ae_decode_hidden(a, a->Z, M)) return rc;
        if (int rc = ae_output(a, M, AE_OUT_TRAIN, x)) return rc;
        if (gauss)
            hipLaunchKernelGGL(ae::ae_elbo_kernel, dim3(1), dim3(256), 0, a->s, a->ll, (int64_t)M * cdiv(g.Dobs, 16),
                               a->kl, (int64_t)M * cdiv(g.Dz, 16), M, a->outs, slot, (double*)nullptr);
        else
            hipLaunchKernelGGL(ae::ae_loglik_kernel, dim3(1), dim3(256), 0, a->s, a->ll, (int64_t)M * cdiv(g.Dobs, 16),
                               M, a->outs, slot);
        CHECK_LAUNCH();
    }
    if (int rc = ae_bwd_decoder(a, R, iw ? ae::B_LATENT_IW : gauss ? ae::B_LATENT
                                         : ae_act_latent(a) ? ae::B_DACT : ae::B_ZPRIOR)) return rc;
    if (iw) {
        hipLaunchKernelGGL(ae::ae_iw_plane_sum_kernel, dim3(cdiv(M * g.Dz, 256)), dim3(256), 0, a->s, a->dmu, a->dlv,
                           M, g.Dz, g.iw_samples);
        CHECK_LAUNCH();
    }
    if (int rc = ae_bwd_encoder(a, xe, M)) return rc;
    if (gauss || ae_corrupting(a)) ++a->step;
    ++a->opt_t;   // one optimiser step, whatever the rule (not the Philox counter above)
    return 0;
}

// ------------------------------------------------------------------ calls over host rows
// The n rows of the host matrix x [n x width] in chunks through xin (core_chunks).
template <class Body>
int ae_chunks(vaeb_ae* a, const float* x, int64_t n, int width, Body body) {
    return core_chunks(a, n, x, width, a->xin, nullptr, 0, nullptr, body);
}

enum AePredict { AE_RECONSTRUCT, AE_ENCODE, AE_DECODE };

// reconstruct / encode / decode over host rows.
int ae_predict(vaeb_ae* a, const float* x, int64_t n, float* out, AePredict what) {
    if (!a || !x || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    const vaeb_ae_config& g = a->c;
    const int win = (what == AE_DECODE) ? g.Dz : g.Dobs;
    const int wout = (what == AE_ENCODE) ? g.Dz : g.Dobs;
    return ae_chunks(a, x, n, win, [&](int64_t r0, int rows) {
        if (what != AE_DECODE)
            if (int rc = ae_encode(a, AeRows{a->xin, rows}, rows, AeNoise{})) return rc;
        if (what != AE_ENCODE) {
            if (int rc = ae_decode_hidden(a, what == AE_DECODE ? a->xin : a->Z, rows)) return rc;
            if (int rc = ae_output(a, rows, AE_OUT_PREDICT)) return rc;
        }
        HIP_TRY(hipMemcpyAsync(out + r0 * wout, what == AE_ENCODE ? a->Z : a->Xpr, sizeof(float) * (size_t)rows * wout,
                               hipMemcpyDeviceToHost, a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
        return 0;
    });
}

}  // namespace

extern "C" {

int vaeb_ae_create(const vaeb_ae_config* cfg, vaeb_ae** out) {
    if (!cfg || !out) return fail(VAEB_ERR_ARG, "null argument");
    const vaeb_ae_config& g = *cfg;
    if (g.Dobs <= 0 || g.Dz <= 0 || g.n_enc < 1 || g.n_dec < 1 || g.n_enc > VAEB_AE_MAX_LAYERS ||
        g.n_dec > VAEB_AE_MAX_LAYERS || g.max_batch <= 0)
        return fail(VAEB_ERR_ARG, "bad autoencoder shape");
    for (int i = 0; i < g.n_enc; ++i) if (g.Denc[i] <= 0) return fail(VAEB_ERR_ARG, "Denc[%d] <= 0", i);
    for (int i = 0; i < g.n_dec; ++i) if (g.Ddec[i] <= 0) return fail(VAEB_ERR_ARG, "Ddec[%d] <= 0", i);
    if (g.otype != VAEB_AE_BINARY && g.otype != VAEB_AE_CONT && g.otype != VAEB_AE_SE)
        return fail(VAEB_ERR_ARG, "otype must be binary|cont|se");
    if (g.act < 0 || g.act > 2) return fail(VAEB_ERR_ARG, "bad activation");
    if (g.latent != VAEB_AE_LATENT_POINT && g.latent != VAEB_AE_LATENT_GAUSS && g.latent != VAEB_AE_LATENT_ACT)
        return fail(VAEB_ERR_ARG, "latent must be VAEB_AE_LATENT_POINT | _GAUSS | _ACT (got %d)", g.latent);
    if (g.otype == VAEB_AE_SE && g.latent == VAEB_AE_LATENT_GAUSS)
        return fail(VAEB_ERR_ARG, "VAEB_AE_SE on a VAEB_AE_LATENT_GAUSS context: -se is no log-likelihood");
    if (!(g.s2 > 0.f) || !(g.eta > 0.f)) return fail(VAEB_ERR_ARG, "s2 and eta must be > 0");
    if (g.iw_samples < 0 || g.iw_samples > (1 << 20))
        return fail(VAEB_ERR_ARG, "iw_samples = %d: 0 to 2^20 (the Philox sample-stream field)", g.iw_samples);
    if (g.iw_samples >= 2 && g.latent != VAEB_AE_LATENT_GAUSS)
        return fail(VAEB_ERR_ARG, "iw_samples = %d needs a VAEB_AE_LATENT_GAUSS context", g.iw_samples);
    if (g.corruption < VAEB_AE_CORRUPT_NONE || g.corruption > VAEB_AE_CORRUPT_GAUSS)
        return fail(VAEB_ERR_ARG, "corruption must be VAEB_AE_CORRUPT_NONE | _MASK | _SALT_PEPPER | _GAUSS (got %d)",
                    g.corruption);
    if (g.prior != VAEB_AE_PRIOR_NORMAL && g.prior != VAEB_AE_PRIOR_TWO_MODE)
        return fail(VAEB_ERR_ARG, "prior must be VAEB_AE_PRIOR_NORMAL | _TWO_MODE (got %d)", g.prior);
    if (g.prior == VAEB_AE_PRIOR_TWO_MODE && g.latent != VAEB_AE_LATENT_GAUSS)
        return fail(VAEB_ERR_ARG, "prior VAEB_AE_PRIOR_TWO_MODE needs a VAEB_AE_LATENT_GAUSS context");
    if (g.corruption != VAEB_AE_CORRUPT_NONE && g.Dobs >= (1 << 30))
        return fail(VAEB_ERR_ARG, "corruption needs Dobs < 2^30 (the Philox c1 field)");
    if (g.corruption != VAEB_AE_CORRUPT_NONE && (int64_t)g.max_batch * g.Dobs >= (1 << 29))
        return fail(VAEB_ERR_ARG, "corruption needs max_batch * Dobs < 2^29 (the corrupted rows' 32-bit byte offsets)");
    auto* a = new vaeb_ae();
    a->c = g;
    for (int i = 0; i < g.n_enc; ++i) { a->enc[i].K = i ? g.Denc[i - 1] : g.Dobs; a->enc[i].N = g.Denc[i]; }
    for (int i = 0; i < g.n_dec; ++i) { a->dec[i].K = i ? g.Ddec[i - 1] : g.Dz; a->dec[i].N = g.Ddec[i]; }
    a->lat.n = ae_gauss(a) ? 2 : 1;              // Wz, or as the cont output: Wzmu, Wzlv
    a->out.n = g.otype == VAEB_AE_CONT ? 2 : 1;  // binary and se: Wout; cont: Wmu, Wlogs2
    for (int j = 0; j < 2; ++j) {
        a->lat.l[j].K = g.Denc[g.n_enc - 1]; a->lat.l[j].N = g.Dz;
        a->out.l[j].K = g.Ddec[g.n_dec - 1]; a->out.l[j].N = g.Dobs;
    }
    // theta order (ae.py:51,56,64,72): encoder, latent, decoder, output; each group's W's, then its b's
    core_place(&a->P, a->enc, g.n_enc);
    core_place(&a->P, a->lat.l, a->lat.n);
    core_place(&a->P, a->dec, g.n_dec);
    core_place(&a->P, a->out.l, a->out.n);
    int rc = core_open(a, g.device, g.eta, g.act, g.max_batch);
    if (rc) { delete a; return rc; }
    const int64_t B = g.max_batch;
    for (int i = 1; i <= g.n_enc; ++i) {
        rc = rc ? rc : a->mem.alloc(&a->H[i], B * a->enc[i - 1].N);
        rc = rc ? rc : a->mem.alloc(&a->dH[i], B * a->enc[i - 1].N);
    }
    for (int i = 1; i <= g.n_dec; ++i) {
        rc = rc ? rc : a->mem.alloc(&a->G[i], B * a->dec[i - 1].N);
        rc = rc ? rc : a->mem.alloc(&a->dG[i], B * a->dec[i - 1].N);
    }
    for (float** p : {&a->Z, &a->dZ}) rc = rc ? rc : a->mem.alloc(p, B * g.Dz);
    // ls2 and dA2 on every output type
    for (float** p : {&a->Xpr, &a->ls2, &a->dA, &a->dA2}) rc = rc ? rc : a->mem.alloc(p, B * g.Dobs);
    rc = rc ? rc : a->mem.alloc(&a->ll, B * cdiv(g.Dobs, 16));
    rc = rc ? rc : a->mem.alloc(&a->xin, B * std::max(g.Dobs, g.Dz));
    if (ae_gauss(a)) {
        for (float** p : {&a->mu, &a->lv, &a->dmu, &a->dlv}) rc = rc ? rc : a->mem.alloc(p, B * g.Dz);
        rc = rc ? rc : a->mem.alloc(&a->kl, B * cdiv(g.Dz, 16));
        rc = rc ? rc : a->mem.alloc(&a->esum, 1);
    }
    if (ae_iw(a)) {
        rc = rc ? rc : ae_iw_scratch(a);
        rc = rc ? rc : a->mem.alloc(&a->iw_wt, B);
        rc = rc ? rc : a->mem.alloc(&a->iw_val, B);
        rc = rc ? rc : a->mem.alloc(&a->iw_lw, B);
    }
    if (ae_corrupting(a)) rc = rc ? rc : a->mem.alloc(&a->xc, B * g.Dobs);
    a->out.d[0] = a->dA; a->out.d[1] = a->dA2;
    a->lat.d[0] = ae_gauss(a) ? a->dmu : a->dZ; a->lat.d[1] = a->dlv;
    if ((rc = core_ready(a, rc))) { delete a; return rc; }
    *out = a;
    return 0;
}

int vaeb_ae_destroy(vaeb_ae* a) {
    if (a) core_close(a);
    delete a;
    return 0;
}

int vaeb_ae_num_params(const vaeb_ae* a, int64_t* n) { return core_num_params(a, n); }

int vaeb_ae_set_data(vaeb_ae* a, const float* x, int64_t n_rows) {
    if (!a || !x || n_rows <= 0) return fail(VAEB_ERR_ARG, "bad data arguments");
    HIP_TRY(hipStreamSynchronize(a->s));
    if (int rc = a->mem.replace(&a->data, n_rows * a->c.Dobs)) return rc;
    HIP_TRY(hipMemcpy(a->data, x, sizeof(float) * (size_t)n_rows * a->c.Dobs, hipMemcpyHostToDevice));
    a->nrows = n_rows;
    return 0;
}

int vaeb_ae_set_params(vaeb_ae* a, const float* f, int64_t n) { return core_xfer(a, a ? a->theta : nullptr, f, nullptr, n); }
int vaeb_ae_get_params(vaeb_ae* a, float* f, int64_t n) { return core_xfer(a, a ? a->theta : nullptr, nullptr, f, n); }
int vaeb_ae_set_adagrad_state(vaeb_ae* a, const float* f, int64_t n) { return core_xfer(a, a ? a->acc : nullptr, f, nullptr, n); }
int vaeb_ae_get_adagrad_state(vaeb_ae* a, float* f, int64_t n) { return core_xfer(a, a ? a->acc : nullptr, nullptr, f, n); }

// ------------------------------------------------------------------ the update rule
int vaeb_ae_set_optimizer(vaeb_ae* a, const vaeb_ae_optimizer* o) { return core_set_optimizer(a, o); }
int vaeb_ae_get_optimizer(vaeb_ae* a, vaeb_ae_optimizer* o) { return core_get_optimizer(a, o); }
int vaeb_ae_set_opt_state(vaeb_ae* a, int32_t slot, const float* f, int64_t n) { return core_opt_state(a, slot, f, nullptr, n); }
int vaeb_ae_get_opt_state(vaeb_ae* a, int32_t slot, float* f, int64_t n) { return core_opt_state(a, slot, nullptr, f, n); }
int vaeb_ae_set_opt_step(vaeb_ae* a, int64_t t) { return core_set_opt_step(a, t); }
int vaeb_ae_get_opt_step(vaeb_ae* a, int64_t* t) { return core_get_opt_step(a, t); }

// The shared checks (core_train_many), then this handle's: the stacked sample planes against
// max_batch, the pushed host eps and corruption noise.
int vaeb_ae_train_many(vaeb_ae* a, const int32_t* idx, int32_t n, int32_t batch, float* out) {
    if (!a) return fail(VAEB_ERR_ARG, "bad arguments");
    auto more = [&]() -> int {
        const bool iw = ae_iw(a);
        if (iw && (int64_t)a->c.iw_samples * std::min(batch, n) > a->c.max_batch)
            return fail(VAEB_ERR_ARG, "iw_samples %d x batch %d > max_batch %d (the stacked sample planes)",
                        a->c.iw_samples, std::min(batch, n), a->c.max_batch);
        if (ae_gauss(a))
            if (int rc = ae_host_eps_ready(a, iw ? (int64_t)a->c.iw_samples * n : (int64_t)n)) return rc;
        return ae_host_corruption_ready(a, n);
    };
    auto step = [a](const int* rows, int m, int slot, int64_t lb, int64_t nn) { return ae_step(a, rows, m, slot, lb, nn); };
    return core_train_many(a, a->data, a->nrows, "vaeb_ae_set_data", idx, n, batch, out, more, step);
}

int vaeb_ae_train(vaeb_ae* a, const int32_t* idx, int32_t n, float* out) {
    if (!a || !idx || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    return vaeb_ae_train_many(a, idx, n, n, out);
}

int vaeb_ae_reconstruct(vaeb_ae* a, const float* x, int64_t n, float* out) { return ae_predict(a, x, n, out, AE_RECONSTRUCT); }
int vaeb_ae_encode(vaeb_ae* a, const float* x, int64_t n, float* z) { return ae_predict(a, x, n, z, AE_ENCODE); }
int vaeb_ae_decode(vaeb_ae* a, const float* z, int64_t n, float* out) { return ae_predict(a, z, n, out, AE_DECODE); }

int vaeb_ae_sq_error(vaeb_ae* a, const float* x, int64_t n, double* out_sum, float* out_rows) {
    if (!a || !x || !out_sum || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    const vaeb_ae_config& g = a->c;
    if (int rc = a->mem.lazy(&a->sq_rows, g.max_batch)) return rc;
    if (int rc = a->mem.lazy(&a->esum, 1)) return rc;
    double total = 0.0;
    if (int rc = ae_chunks(a, x, n, g.Dobs, [&](int64_t r0, int rows) {
            // the deterministic forward (Gaussian latent: z = mu), then the mean head's (Y - P)^2 partials
            const AeRows xc{a->xin, rows};
            if (int rc = ae_encode(a, xc, rows, AeNoise{})) return rc;
            if (int rc = ae_decode_hidden(a, a->Z, rows)) return rc;
            if (int rc = ae_output(a, rows, AE_OUT_SQ, xc)) return rc;
            hipLaunchKernelGGL(ae::ae_row_sum_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, a->s, a->ll, rows,
                               cdiv(g.Dobs, 16), a->sq_rows);
            CHECK_LAUNCH();
            return core_sum_to_host(a, a->sq_rows, rows, &total, out_rows ? out_rows + r0 : nullptr);
        })) return rc;
    *out_sum = total;
    return 0;
}

// ------------------------------------------------------------------ Gaussian latent
#define AE_NEED_GAUSS(a, fn)                                                                            \
    do {                                                                                                \
        if (!(a)) return fail(VAEB_ERR_ARG, "null argument");                                           \
        if (!ae_gauss(a)) return fail(VAEB_ERR_ARG, fn " needs a VAEB_AE_LATENT_GAUSS context");        \
    } while (0)

// the step counter: Gaussian-latent and corrupting contexts draw at it
#define AE_NEED_STEP(a, fn)                                                                             \
    do {                                                                                                \
        if (!(a)) return fail(VAEB_ERR_ARG, "null argument");                                           \
        if (!ae_gauss(a) && !ae_corrupting(a))                                                          \
            return fail(VAEB_ERR_ARG, fn " needs a VAEB_AE_LATENT_GAUSS or a corrupting context");      \
    } while (0)
#define AE_NEED_CORRUPT(a, fn)                                                                          \
    do {                                                                                                \
        if (!(a)) return fail(VAEB_ERR_ARG, "null argument");                                           \
        if (!ae_corrupting(a)) return fail(VAEB_ERR_ARG, fn " needs a context created with a corruption"); \
    } while (0)

int vaeb_ae_set_eps_mode(vaeb_ae* a, int32_t mode, uint64_t seed) {
    AE_NEED_GAUSS(a, "vaeb_ae_set_eps_mode");
    if (mode != VAEB_EPS_PHILOX && mode != VAEB_EPS_HOST) return fail(VAEB_ERR_ARG, "bad eps mode");
    HIP_TRY(hipStreamSynchronize(a->s));
    a->eps_mode = mode;
    a->seed = seed;
    return 0;
}

int vaeb_ae_push_eps(vaeb_ae* a, const float* eps, int64_t rows) {
    AE_NEED_GAUSS(a, "vaeb_ae_push_eps");
    if (!eps || rows <= 0) return fail(VAEB_ERR_ARG, "bad eps arguments");
    const int64_t n = rows * a->c.Dz;
    HIP_TRY(hipStreamSynchronize(a->s));
    if (n > a->eps_cap) a->eps_rows = 0;   // the old rows go with the old buffer
    if (int rc = a->mem.grow(&a->eps_in, &a->eps_cap, n)) return rc;
    HIP_TRY(hipMemcpy(a->eps_in, eps, sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
    a->eps_rows = rows;
    return 0;
}

int vaeb_ae_set_step(vaeb_ae* a, int64_t step) {
    AE_NEED_STEP(a, "vaeb_ae_set_step");
    a->step = step;
    return 0;
}

int vaeb_ae_get_step(vaeb_ae* a, int64_t* step) {
    AE_NEED_STEP(a, "vaeb_ae_get_step");
    if (!step) return fail(VAEB_ERR_ARG, "null argument");
    *step = a->step;
    return 0;
}

int vaeb_ae_encode_dist(vaeb_ae* a, const float* x, int64_t n, float* out_mu, float* out_lv, float* out_z) {
    AE_NEED_GAUSS(a, "vaeb_ae_encode_dist");
    if (!x || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    const vaeb_ae_config& g = a->c;
    if (out_z)
        if (int rc = ae_host_eps_ready(a, n)) return rc;
    return ae_chunks(a, x, n, g.Dobs, [&](int64_t r0, int rows) {
        if (int rc = ae_encode(a, AeRows{a->xin, rows}, rows, AeNoise{out_z ? AE_EPS_EVAL : AE_EPS_ZERO, nullptr, r0}))
            return rc;
        const size_t nb = sizeof(float) * (size_t)rows * g.Dz;
        if (out_mu) HIP_TRY(hipMemcpyAsync(out_mu + r0 * g.Dz, a->mu, nb, hipMemcpyDeviceToHost, a->s));
        if (out_lv) HIP_TRY(hipMemcpyAsync(out_lv + r0 * g.Dz, a->lv, nb, hipMemcpyDeviceToHost, a->s));
        if (out_z) HIP_TRY(hipMemcpyAsync(out_z + r0 * g.Dz, a->Z, nb, hipMemcpyDeviceToHost, a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
        return 0;
    });
}

int vaeb_ae_elbo(vaeb_ae* a, const float* x, int64_t n, double* out_sum) {
    AE_NEED_GAUSS(a, "vaeb_ae_elbo");
    if (!x || !out_sum || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    const vaeb_ae_config& g = a->c;
    if (int rc = ae_host_eps_ready(a, n)) return rc;
    double total = 0.0;
    if (int rc = ae_chunks(a, x, n, g.Dobs, [&](int64_t r0, int rows) {
            const AeRows xc{a->xin, rows};
            if (int rc = ae_encode(a, xc, rows, AeNoise{AE_EPS_EVAL, nullptr, r0})) return rc;
            if (int rc = ae_decode_hidden(a, a->Z, rows)) return rc;
            if (int rc = ae_output(a, rows, AE_OUT_TRAIN, xc)) return rc;
            // writes esum itself: no memset
            hipLaunchKernelGGL(ae::ae_elbo_kernel, dim3(1), dim3(256), 0, a->s, a->ll, (int64_t)rows * cdiv(g.Dobs, 16),
                               a->kl, (int64_t)rows * cdiv(g.Dz, 16), rows, (float*)nullptr, 0, a->esum);
            CHECK_LAUNCH();
            return core_sum_to_host(a, nullptr, 0, &total);
        })) return rc;
    *out_sum = total;
    return 0;
}

int vaeb_ae_marginal_ll(vaeb_ae* a, const float* x, int64_t n, int32_t K, double* out_sum, float* out_rows) {
    AE_NEED_GAUSS(a, "vaeb_ae_marginal_ll");
    if (!x || !out_sum || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (K < 1 || K > (1 << 20))
        return fail(VAEB_ERR_ARG, "K = %d: 1 to 2^20 samples (the Philox sample-stream field)", K);
    if (int rc = ae_host_eps_ready(a, n * K)) return rc;
    const vaeb_ae_config& g = a->c;
    const int B = g.max_batch;
    if (int rc = ae_iw_scratch(a)) return rc;
    IwArgs w{};
    w.nctD = cdiv(g.Dobs, 16); w.K = K; w.logK = (float)std::log((double)K);
    w.lat = a->iw; w.ms = a->iw + B; w.rows = a->iw + 3 * (int64_t)B; w.lp_part = a->ll;
    ae::AeIwArgs q{};
    q.Dz = g.Dz; q.n = n;
    q.eps_mode = a->eps_mode == VAEB_EPS_HOST ? 1 : 0;
    q.seed = a->seed; q.step = a->step; q.eps_in = a->eps_in;
    q.mu = a->mu; q.lv = a->lv; q.z = a->Z; q.lat = a->iw; q.yrow = a->iw_yrow;
    double total = 0.0;
    if (int rc = ae_chunks(a, x, n, g.Dobs, [&](int64_t r0, int R) {
            if (int rc = ae_encode(a, AeRows{a->xin, R}, R, AeNoise{})) return rc;   // mu, lv: once
            const int smax = std::max(1, B / R);   // sample planes per pass: S * R <= max_batch stacked rows
            w.Mb = w.Mbp = q.R = R;
            q.row0 = r0;
            for (int k0 = 0; k0 < K; k0 += smax) {
                const int S = std::min(smax, K - k0);
                w.k0 = q.k0 = k0; w.S = q.S = S;
                if (int rc = ae_iw_sample(a, q, S * R)) return rc;
                if (int rc = ae_decode_hidden(a, a->Z, S * R)) return rc;
                if (int rc = ae_output(a, S * R, AE_OUT_VALUE, AeRows{a->xin, R, a->iw_yrow})) return rc;
                hipLaunchKernelGGL(iw_lse_kernel, dim3(cdiv(R, 256)), dim3(256), 0, a->s, w);
                CHECK_LAUNCH();
            }
            return core_sum_to_host(a, w.rows, R, &total, out_rows ? out_rows + r0 : nullptr);
        })) return rc;
    *out_sum = total;
    return 0;
}
#undef AE_NEED_GAUSS
#undef AE_NEED_STEP

// ------------------------------------------------------------------ two-mode latent prior
#define AE_NEED_TWO_MODE(a, fn)                                                                         \
    do {                                                                                                \
        if (!(a)) return fail(VAEB_ERR_ARG, "null argument");                                           \
        if (!ae_two_mode(a)) return fail(VAEB_ERR_ARG, fn " needs a context created with VAEB_AE_PRIOR_TWO_MODE"); \
    } while (0)

int vaeb_ae_set_prior(vaeb_ae* a, float mean1, float width) {
    AE_NEED_TWO_MODE(a, "vaeb_ae_set_prior");
    if (!(std::fabs(mean1) <= 1e3f) || !(width >= 1e-3f && width <= 1e3f))   // NaN fails both
        return fail(VAEB_ERR_ARG, "prior mean1 %g, width %g: |mean1| <= 1e3 and 1e-3 <= width <= 1e3", (double)mean1,
                    (double)width);
    a->pr_mean1 = mean1; a->pr_width = width;   // launch arguments: the enqueued steps keep theirs
    return 0;
}

int vaeb_ae_get_prior(vaeb_ae* a, float* mean1, float* width) {
    AE_NEED_TWO_MODE(a, "vaeb_ae_get_prior");
    if (!mean1 || !width) return fail(VAEB_ERR_ARG, "null argument");
    *mean1 = a->pr_mean1; *width = a->pr_width;
    return 0;
}

int vaeb_ae_encode_bits(vaeb_ae* a, const float* x, int64_t n, uint32_t* out_words) {
    AE_NEED_TWO_MODE(a, "vaeb_ae_encode_bits");
    if (!x || !out_words || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    const vaeb_ae_config& g = a->c;
    const int nw = cdiv(g.Dz, 32);
    if (int rc = a->mem.lazy(&a->code_w, (int64_t)g.max_batch * nw)) return rc;
    return ae_chunks(a, x, n, g.Dobs, [&](int64_t r0, int rows) {
        if (int rc = ae_encode(a, AeRows{a->xin, rows}, rows, AeNoise{})) return rc;   // vaeb_ae_encode's mu
        hipLaunchKernelGGL(ae::ae_pack_bits_kernel, dim3(cdiv(rows * nw, 256)), dim3(256), 0, a->s, a->mu, rows, g.Dz,
                           0.5f * a->pr_mean1, a->code_w);
        CHECK_LAUNCH();
        HIP_TRY(hipMemcpyAsync(out_words + r0 * nw, a->code_w, sizeof(uint32_t) * (size_t)rows * nw,
                               hipMemcpyDeviceToHost, a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
        return 0;
    });
}

int vaeb_ae_decode_bits(vaeb_ae* a, const uint32_t* words, int64_t n, float* out) {
    AE_NEED_TWO_MODE(a, "vaeb_ae_decode_bits");
    if (!words || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    const vaeb_ae_config& g = a->c;
    const int nw = cdiv(g.Dz, 32);
    // the chunk loop uploads 4-byte elements, whatever they hold: nw words per row into xin (>= Dz per row)
    return ae_chunks(a, reinterpret_cast<const float*>(words), n, nw, [&](int64_t r0, int rows) {
        hipLaunchKernelGGL(ae::ae_unpack_bits_kernel, dim3(cdiv(rows * g.Dz, 256)), dim3(256), 0, a->s,
                           reinterpret_cast<const uint32_t*>(a->xin), rows, g.Dz, a->pr_mean1, a->Z);
        CHECK_LAUNCH();
        if (int rc = ae_decode_hidden(a, a->Z, rows)) return rc;   // vaeb_ae_decode's launches on z in {0, a}
        if (int rc = ae_output(a, rows, AE_OUT_PREDICT)) return rc;
        HIP_TRY(hipMemcpyAsync(out + r0 * g.Dobs, a->Xpr, sizeof(float) * (size_t)rows * g.Dobs, hipMemcpyDeviceToHost,
                               a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
        return 0;
    });
}
#undef AE_NEED_TWO_MODE

// ------------------------------------------------------------------ input corruption
int vaeb_ae_set_corruption_level(vaeb_ae* a, float level) {
    AE_NEED_CORRUPT(a, "vaeb_ae_set_corruption_level");
    const bool unit = a->c.corruption != VAEB_AE_CORRUPT_GAUSS;
    if (!(level >= 0.f) || (unit ? level > 1.f : !std::isfinite(level)))   // NaN fails the first
        return fail(VAEB_ERR_ARG, unit ? "corruption level %g: 0 to 1" : "corruption level %g: finite and >= 0", (double)level);
    a->cor_level = level;   // a launch argument: the enqueued steps keep theirs
    return 0;
}

int vaeb_ae_get_corruption_level(vaeb_ae* a, float* out) {
    AE_NEED_CORRUPT(a, "vaeb_ae_get_corruption_level");
    if (!out) return fail(VAEB_ERR_ARG, "null argument");
    *out = a->cor_level;
    return 0;
}

int vaeb_ae_set_corruption_noise(vaeb_ae* a, int32_t mode, uint64_t seed) {
    AE_NEED_CORRUPT(a, "vaeb_ae_set_corruption_noise");
    if (mode != VAEB_EPS_PHILOX && mode != VAEB_EPS_HOST) return fail(VAEB_ERR_ARG, "bad corruption noise mode");
    HIP_TRY(hipStreamSynchronize(a->s));
    a->cor_mode = mode;
    a->cor_seed = seed;
    return 0;
}

int vaeb_ae_push_corruption(vaeb_ae* a, const float* r, int64_t rows) {
    AE_NEED_CORRUPT(a, "vaeb_ae_push_corruption");
    if (!r || rows <= 0) return fail(VAEB_ERR_ARG, "bad corruption noise arguments");
    const int64_t n = rows * a->c.Dobs;
    HIP_TRY(hipStreamSynchronize(a->s));
    if (n > a->cor_cap) a->cor_rows = 0;   // the old rows go with the old buffer
    if (int rc = a->mem.grow(&a->cor_in, &a->cor_cap, n)) return rc;
    HIP_TRY(hipMemcpy(a->cor_in, r, sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
    a->cor_rows = rows;
    return 0;
}

int vaeb_ae_corrupt(vaeb_ae* a, const int32_t* idx, int32_t n, float* out) {
    AE_NEED_CORRUPT(a, "vaeb_ae_corrupt");
    if (!idx || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = core_check_idx(a->data, a->nrows, "vaeb_ae_set_data", idx, n)) return rc;
    if (int rc = ae_host_corruption_ready(a, n)) return rc;
    if (int rc = core_reserve(a, n, 1)) return rc;
    const int D = a->c.Dobs;
    HIP_TRY(hipMemcpyAsync(a->idx, idx, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, a->s));
    for (int64_t lb = 0; lb < n; lb += a->c.max_batch) {
        const int m = (int)std::min<int64_t>(a->c.max_batch, n - lb);
        if (int rc = ae_corrupt_rows(a, a->idx + lb, m, lb)) return rc;
        HIP_TRY(hipMemcpyAsync(out + lb * D, a->xc, sizeof(float) * (size_t)m * D, hipMemcpyDeviceToHost, a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
    }
    return 0;
}
#undef AE_NEED_CORRUPT

}  // extern "C"
