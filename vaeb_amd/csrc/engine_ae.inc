// engine_ae.inc -- the degenerate-vae autoencoder (include/vaeb_hip.h vaeb_ae_*) on the
// fp32 tile engine (ae_mlp.hpp).  Included by vaeb_hip.hip after the VAEB helpers.

struct vaeb_ae {
    vaeb_ae_config c{};
    hipStream_t s = nullptr;
    std::vector<int> de, dd;          // encoder dims [Dobs, Denc...], decoder dims [Dz, Ddec...]
    int64_t P = 0;
    std::vector<int64_t> oWe, obe, oWd, obd;
    int64_t oWz = 0, obz = 0, oWo = 0, obo = 0, oWl = 0, obl = 0;   // out: Wout/bout or Wmu/bmu (+ Wlogs2/blogs2)
    int64_t oWzl = 0, obzl = 0;       // Gaussian latent: oWz / obz = Wzmu / bzmu, these = Wzlv / bzlv
    float *theta = nullptr, *acc = nullptr;
    float* data = nullptr;
    int64_t nrows = 0;
    int* idx = nullptr;               // device index list (epoch capacity)
    int idx_cap = 0;
    std::vector<float*> H, G, dH, dG; // activations / deltas per layer (H[0], G[0] unused)
    float *Z = nullptr, *dZ = nullptr, *Xpr = nullptr, *ls2 = nullptr, *dA = nullptr, *dA2 = nullptr;
    float *ll = nullptr, *outs = nullptr, *xin = nullptr;
    int outs_cap = 0;
    // Gaussian latent (c.latent == VAEB_AE_LATENT_GAUSS): a->Z holds z
    float *mu = nullptr, *lv = nullptr, *dmu = nullptr, *dlv = nullptr, *kl = nullptr;
    double* esum = nullptr;           // vaeb_ae_elbo / vaeb_ae_marginal_ll / vaeb_ae_sq_error: one chunk's sum
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
};

namespace {

int ae_alloc(float** p, int64_t n) { return dalloc(p, (size_t)std::max<int64_t>(n, 1)); }

bool ae_gauss(const vaeb_ae* a) { return a->c.latent == VAEB_AE_LATENT_GAUSS; }
bool ae_act_latent(const vaeb_ae* a) { return a->c.latent == VAEB_AE_LATENT_ACT; }
bool ae_iw(const vaeb_ae* a) { return a->c.iw_samples >= 2; }

// vaeb_ae_marginal_ll's and the importance-weighted step's scratch, sized by max_batch
int ae_iw_scratch(vaeb_ae* a) {
    const int64_t B = a->c.max_batch;
    if (!a->iw)
        if (int rc = ae_alloc(&a->iw, 4 * B)) return rc;
    if (!a->iw_yrow)
        if (int rc = dalloc(&a->iw_yrow, (size_t)B)) return rc;
    return 0;
}

// eps of one latent forward (ae::PAeFwd F_LATENT): zero (the deterministic predictions),
// rows of the pushed host eps, or Philox keyed by rows[m] / row0 + m, the step and the domain.
struct AeNoise {
    int mode = ae::NOISE_ZERO;
    const float* eps = nullptr;
    const int* rows = nullptr;
    uint32_t row0 = 0;
    int64_t step = 0;
    uint32_t domain = 0;
};

// The noise of rows [r0, r0 + ...) of a call in the context's eps mode: training (domain 0,
// keyed by the dataset rows idx) or evaluation (domain 1, stream 0, keyed by r0 + m).
AeNoise ae_noise(const vaeb_ae* a, const int* idx, int64_t r0, int64_t step, bool eval) {
    AeNoise z;
    if (a->eps_mode == VAEB_EPS_HOST) {
        z.mode = ae::NOISE_HOST;
        z.eps = a->eps_in + r0 * a->c.Dz;
    } else {
        z.mode = ae::NOISE_PHILOX;
        z.rows = idx;
        z.row0 = (uint32_t)r0;
        z.step = step;
        z.domain = eval ? 1u : 0u;
    }
    return z;
}

int ae_host_eps_ready(const vaeb_ae* a, int64_t rows) {
    if (a->eps_mode == VAEB_EPS_HOST && a->eps_rows != rows)
        return fail(VAEB_ERR_STATE, "host eps mode: pushed %lld rows, the call needs %lld (call vaeb_ae_push_eps)",
                    (long long)a->eps_rows, (long long)rows);
    return 0;
}

// Forward through the whole network for M rows: in[ri] (ri = idx[m] when idx != null),
// Y (observations for the loglik / deltas, nullptr for predictions), stop_at_z: encode only.
// value_only (with train and zin): the output layer leaves the loglik partials and nothing else.
// sq (with train; vaeb_ae_sq_error): the output layer is the value-only squared error of the mean
// head, whatever the context's otype.
int ae_forward(vaeb_ae* a, const float* in, int in_rows, const int* idx, int M, bool train, bool stop_at_z,
               const float* zin, const AeNoise& nz = AeNoise{}, bool value_only = false, bool sq = false) {
    const vaeb_ae_config& g = a->c;
    hipStream_t s = a->s;
    const int ne = g.n_enc, nd = g.n_dec;
    if (!zin) {
        for (int i = 0; i < ne; ++i) {
            ae::PAeFwd p{};
            p.M = M; p.N = a->de[i + 1]; p.K = a->de[i];
            p.in = (i == 0) ? in : a->H[i]; p.ldin = a->de[i]; p.in_rows = (i == 0) ? in_rows : M;
            p.idx = (i == 0) ? idx : nullptr;
            p.W = a->theta + a->oWe[i]; p.b = a->theta + a->obe[i];
            p.mode = ae::F_ACT; p.act = g.act; p.out = a->H[i + 1];
            launch_bigk<1>(s, p);
            CHECK_LAUNCH();
        }
        ae::PAeFwd p{};
        p.M = M; p.N = g.Dz; p.K = a->de[ne];
        p.in = a->H[ne]; p.ldin = a->de[ne]; p.in_rows = M;
        p.W = a->theta + a->oWz; p.b = a->theta + a->obz;
        if (ae_gauss(a)) {
            p.W2 = a->theta + a->oWzl; p.b2 = a->theta + a->obzl;
            p.mode = ae::F_LATENT; p.out = a->mu; p.out2 = a->lv; p.zout = a->Z;
            p.llpart = a->kl; p.nct = cdiv(g.Dz, 16);
            p.noise = nz.mode; p.eps_in = nz.eps; p.erow = nz.rows; p.erow0 = nz.row0;
            p.seed = a->seed; p.step = nz.step; p.domain = nz.domain;
            launch_bigk<2>(s, p);
        } else {   // Z = H Wz + bz, or f of it (the activated latent)
            p.mode = ae_act_latent(a) ? ae::F_ACT : ae::F_LINEAR; p.act = g.act; p.out = a->Z;
            launch_bigk<1>(s, p);
        }
        CHECK_LAUNCH();
        if (stop_at_z) return 0;
    }
    for (int i = 0; i < nd; ++i) {
        ae::PAeFwd p{};
        p.M = M; p.N = a->dd[i + 1]; p.K = a->dd[i];
        p.in = (i == 0) ? (zin ? zin : a->Z) : a->G[i]; p.ldin = a->dd[i]; p.in_rows = M;
        p.W = a->theta + a->oWd[i]; p.b = a->theta + a->obd[i];
        p.mode = ae::F_ACT; p.act = g.act; p.out = a->G[i + 1];
        launch_bigk<1>(s, p);
        CHECK_LAUNCH();
    }
    if (train && (sq || g.otype == VAEB_AE_SE)) {   // squared error: its own instantiation
        ae::PAeFwdSe p{};
        p.M = M; p.N = g.Dobs; p.K = a->dd[nd];
        p.in = a->G[nd]; p.ldin = a->dd[nd]; p.in_rows = M;
        p.W = a->theta + a->oWo; p.b = a->theta + a->obo;   // cont: the mean head Wmu / bmu alone
        p.out = a->Xpr;
        p.Y = in; p.yidx = idx; p.ldy = g.Dobs; p.y_rows = in_rows;
        p.dA = (sq || value_only) ? nullptr : a->dA; p.llpart = a->ll; p.nct = cdiv(g.Dobs, 16);
        p.mode = ae::F_OUT_SE;
        launch_bigk<1>(s, p);
        CHECK_LAUNCH();
        return 0;
    }
    ae::PAeFwd p{};
    p.M = M; p.N = g.Dobs; p.K = a->dd[nd];
    p.in = a->G[nd]; p.ldin = a->dd[nd]; p.in_rows = M;
    p.W = a->theta + a->oWo; p.b = a->theta + a->obo;
    p.out = a->Xpr;
    if (train) { p.Y = in; p.yidx = idx; p.ldy = g.Dobs; p.y_rows = in_rows; }
    p.dA = value_only ? nullptr : a->dA; p.llpart = a->ll; p.nct = cdiv(g.Dobs, 16);
    if (g.otype != VAEB_AE_CONT) {   // binary, and the predictions (no Y) of a squared-error context
        p.mode = ae::F_OUT_BIN;
        launch_bigk<1>(s, p);
    } else {
        p.mode = ae::F_OUT_CONT;
        p.W2 = a->theta + a->oWl; p.b2 = a->theta + a->obl; p.out2 = a->ls2;
        p.dA2 = value_only ? nullptr : a->dA2;
        launch_bigk<2>(s, p);
    }
    CHECK_LAUNCH();
    return 0;
}

// One weight-gradient + AdaGrad launch for W [Kin x N] / b [N] from in (gathered through
// idx for the first layer) and the layer's output delta.
int ae_wgrad(vaeb_ae* a, const float* in, int in_rows, const int* idx, int Kin, const float* dout, int N, int M,
             int64_t offW, int64_t offb) {
    ae::PAeWgrad p{};
    p.M = Kin + 1; p.N = N; p.K = M;
    p.in = in; p.ldin = Kin; p.in_rows = in_rows; p.idx = idx; p.Kin = Kin;
    p.dout = dout;
    p.theta = a->theta; p.accum = a->acc; p.offW = offW; p.offb = offb;
    p.eta = a->c.eta; p.inv_s2 = 1.0f / a->c.s2;
    launch_bigk<1>(a->s, p);
    CHECK_LAUNCH();
    return 0;
}

template <bool IW = false>
int ae_bwd(vaeb_ae* a, const float* dout, const float* dout2, int K1, const float* W, const float* W2, int N, int M,
           const float* h, int mode, float* din) {
    ae::PAeBwdT<IW> p{};
    p.M = M; p.N = N; p.K = dout2 ? 2 * K1 : K1;
    p.dout = dout; p.dout2 = dout2; p.K1 = K1; p.W = W; p.W2 = W2;
    p.h = h; p.mode = mode; p.act = a->c.act; p.din = din;
    if (mode == ae::B_LATENT || mode == ae::B_LATENT_IW) {
        p.h = a->mu; p.h2 = a->lv; p.h3 = a->Z; p.din = a->dmu; p.din2 = a->dlv;
    }
    if constexpr (IW) { p.wt = a->iw_wt; p.Mp = M / a->c.iw_samples; }
    launch_bigk<1>(a->s, p);
    CHECK_LAUNCH();
    return 0;
}

// train(idx): forward + loglik, then per layer (output first) the data gradient with the
// old weights followed by the weight update of that layer.  loglik / M -> outs[slot]
// (Gaussian latent: (loglik - KL) / M, eps from nz; one launch more, the lv head's wgrad).
// Squared-error output: the partials are se, so outs[slot] = se / M (positive) while the deltas
// are those of -se.  Activated latent: the decoder's first data gradient is times f'(Z), no - Z.
int ae_step(vaeb_ae* a, const int* idx, int M, int slot, const AeNoise& nz = AeNoise{}) {
    const vaeb_ae_config& g = a->c;
    const int ne = g.n_enc, nd = g.n_dec, D = g.Dobs;
    const bool cont = g.otype == VAEB_AE_CONT, gauss = ae_gauss(a);
    if (int rc = ae_forward(a, a->data, (int)a->nrows, idx, M, true, false, nullptr, nz)) return rc;
    if (gauss)
        hipLaunchKernelGGL(ae::ae_elbo_kernel, dim3(1), dim3(256), 0, a->s, a->ll, (int64_t)M * cdiv(D, 16), a->kl,
                           (int64_t)M * cdiv(g.Dz, 16), M, a->outs, slot, (double*)nullptr);
    else
        hipLaunchKernelGGL(ae::ae_loglik_kernel, dim3(1), dim3(256), 0, a->s, a->ll, (int64_t)M * cdiv(D, 16), M,
                           a->outs, slot);
    CHECK_LAUNCH();
    // output layer
    const int Hd = a->dd[nd];
    if (int rc = ae_bwd(a, a->dA, cont ? a->dA2 : nullptr, D, a->theta + a->oWo, cont ? a->theta + a->oWl : nullptr,
                        Hd, M, a->G[nd], ae::B_DACT, a->dG[nd])) return rc;
    if (int rc = ae_wgrad(a, a->G[nd], M, nullptr, Hd, a->dA, D, M, a->oWo, a->obo)) return rc;
    if (cont)
        if (int rc = ae_wgrad(a, a->G[nd], M, nullptr, Hd, a->dA2, D, M, a->oWl, a->obl)) return rc;
    // decoder layers (top down): dG[i+1] is the pre-activation delta of layer i
    for (int i = nd - 1; i >= 0; --i) {
        const float* hin = (i == 0) ? a->Z : a->G[i];
        float* dst = (i == 0) ? a->dZ : a->dG[i];
        if (int rc = ae_bwd(a, a->dG[i + 1], nullptr, a->dd[i + 1], a->theta + a->oWd[i], nullptr, a->dd[i], M, hin,
                            i == 0 ? (gauss ? ae::B_LATENT : ae_act_latent(a) ? ae::B_DACT : ae::B_ZPRIOR)
                                   : ae::B_DACT, dst)) return rc;
        if (int rc = ae_wgrad(a, hin, M, nullptr, a->dd[i], a->dG[i + 1], a->dd[i + 1], M, a->oWd[i], a->obd[i]))
            return rc;
    }
    // latent layer Z = H W z + bz (dZ: its pre-activation delta on the activated latent), or the two heads [mu | lv] = H [Wzmu | Wzlv] + [bzmu | bzlv]
    if (gauss) {
        if (int rc = ae_bwd(a, a->dmu, a->dlv, g.Dz, a->theta + a->oWz, a->theta + a->oWzl, a->de[ne], M, a->H[ne],
                            ae::B_DACT, a->dH[ne])) return rc;
        if (int rc = ae_wgrad(a, a->H[ne], M, nullptr, a->de[ne], a->dmu, g.Dz, M, a->oWz, a->obz)) return rc;
        if (int rc = ae_wgrad(a, a->H[ne], M, nullptr, a->de[ne], a->dlv, g.Dz, M, a->oWzl, a->obzl)) return rc;
    } else {
        if (int rc = ae_bwd(a, a->dZ, nullptr, g.Dz, a->theta + a->oWz, nullptr, a->de[ne], M, a->H[ne], ae::B_DACT,
                            a->dH[ne])) return rc;
        if (int rc = ae_wgrad(a, a->H[ne], M, nullptr, a->de[ne], a->dZ, g.Dz, M, a->oWz, a->obz)) return rc;
    }
    // encoder layers (top down); no data gradient into X
    for (int i = ne - 1; i >= 0; --i) {
        if (i > 0)
            if (int rc = ae_bwd(a, a->dH[i + 1], nullptr, a->de[i + 1], a->theta + a->oWe[i], nullptr, a->de[i], M,
                                a->H[i], ae::B_DACT, a->dH[i])) return rc;
        const float* in = (i == 0) ? a->data : a->H[i];
        if (int rc = ae_wgrad(a, in, i == 0 ? (int)a->nrows : M, i == 0 ? idx : nullptr, a->de[i], a->dH[i + 1],
                              a->de[i + 1], M, a->oWe[i], a->obe[i])) return rc;
    }
    return 0;
}

// train(idx) on the K-sample importance-weighted bound (c.iw_samples = K >= 2, ae_iwae.hpp): the
// encoder once on the M rows, the decoder forward and backward on the K * M stacked rows
// (g = k * M + m) with the output deltas scaled by the normalised weights, the K planes of
// dmu / dlv summed, then the encoder's backward on M rows as in ae_step.  L_K / M -> outs[slot].
// lb: the step's offset in the call's idx list of n rows (host eps: sample k of list position i
// at row k * n + i).
int ae_step_iw(vaeb_ae* a, const int* idx, int M, int slot, int64_t lb, int64_t n, int64_t step) {
    const vaeb_ae_config& g = a->c;
    const int ne = g.n_enc, nd = g.n_dec, D = g.Dobs, K = g.iw_samples, KM = K * M;
    const bool cont = g.otype == VAEB_AE_CONT;
    if (int rc = ae_forward(a, a->data, (int)a->nrows, idx, M, false, true, nullptr)) return rc;   // mu, lv
    ae::AeIwArgs q{};
    q.Dz = g.Dz; q.R = M; q.S = K; q.k0 = 0; q.row0 = lb; q.n = n;
    q.eps_mode = a->eps_mode == VAEB_EPS_HOST ? 1 : 0;
    q.seed = a->seed; q.step = step; q.eps_in = a->eps_in;
    q.mu = a->mu; q.lv = a->lv; q.z = a->Z; q.lat = a->iw; q.yrow = a->iw_yrow; q.idx = idx;
    hipLaunchKernelGGL(ae::ae_iw_sample_kernel, dim3(cdiv(KM, 16)), dim3(256), 0, a->s, q);
    CHECK_LAUNCH();
    if (int rc = ae_forward(a, a->data, (int)a->nrows, a->iw_yrow, KM, true, false, a->Z)) return rc;
    ae::AeIwWeightArgs w{};
    w.M = M; w.K = K; w.D = D; w.nct = cdiv(D, 16); w.logK = std::log((double)K);
    w.llpart = a->ll; w.lat = a->iw; w.lw = a->iw_lw; w.wt = a->iw_wt; w.rowval = a->iw_val;
    w.dA = a->dA; w.dA2 = cont ? a->dA2 : nullptr;
    hipLaunchKernelGGL(ae::ae_iw_weight_kernel, dim3(M), dim3(256), 0, a->s, w);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(ae::ae_loglik_kernel, dim3(1), dim3(256), 0, a->s, a->iw_val, (int64_t)M, M, a->outs, slot);
    CHECK_LAUNCH();
    // output layer and decoder on the stacked rows
    const int Hd = a->dd[nd];
    if (int rc = ae_bwd(a, a->dA, cont ? a->dA2 : nullptr, D, a->theta + a->oWo, cont ? a->theta + a->oWl : nullptr,
                        Hd, KM, a->G[nd], ae::B_DACT, a->dG[nd])) return rc;
    if (int rc = ae_wgrad(a, a->G[nd], KM, nullptr, Hd, a->dA, D, KM, a->oWo, a->obo)) return rc;
    if (cont)
        if (int rc = ae_wgrad(a, a->G[nd], KM, nullptr, Hd, a->dA2, D, KM, a->oWl, a->obl)) return rc;
    for (int i = nd - 1; i >= 0; --i) {
        const float* hin = (i == 0) ? a->Z : a->G[i];
        if (int rc = i == 0 ? ae_bwd<true>(a, a->dG[1], nullptr, a->dd[1], a->theta + a->oWd[0], nullptr, a->dd[0], KM,
                                           hin, ae::B_LATENT_IW, nullptr)
                            : ae_bwd(a, a->dG[i + 1], nullptr, a->dd[i + 1], a->theta + a->oWd[i], nullptr, a->dd[i], KM,
                                     hin, ae::B_DACT, a->dG[i])) return rc;
        if (int rc = ae_wgrad(a, hin, KM, nullptr, a->dd[i], a->dG[i + 1], a->dd[i + 1], KM, a->oWd[i], a->obd[i]))
            return rc;
    }
    hipLaunchKernelGGL(ae::ae_iw_plane_sum_kernel, dim3(cdiv(M * g.Dz, 256)), dim3(256), 0, a->s, a->dmu, a->dlv, M,
                       g.Dz, K);
    CHECK_LAUNCH();
    // the two heads and the encoder on the M rows, as ae_step
    if (int rc = ae_bwd(a, a->dmu, a->dlv, g.Dz, a->theta + a->oWz, a->theta + a->oWzl, a->de[ne], M, a->H[ne],
                        ae::B_DACT, a->dH[ne])) return rc;
    if (int rc = ae_wgrad(a, a->H[ne], M, nullptr, a->de[ne], a->dmu, g.Dz, M, a->oWz, a->obz)) return rc;
    if (int rc = ae_wgrad(a, a->H[ne], M, nullptr, a->de[ne], a->dlv, g.Dz, M, a->oWzl, a->obzl)) return rc;
    for (int i = ne - 1; i >= 0; --i) {
        if (i > 0)
            if (int rc = ae_bwd(a, a->dH[i + 1], nullptr, a->de[i + 1], a->theta + a->oWe[i], nullptr, a->de[i], M,
                                a->H[i], ae::B_DACT, a->dH[i])) return rc;
        const float* in = (i == 0) ? a->data : a->H[i];
        if (int rc = ae_wgrad(a, in, i == 0 ? (int)a->nrows : M, i == 0 ? idx : nullptr, a->de[i], a->dH[i + 1],
                              a->de[i + 1], M, a->oWe[i], a->obe[i])) return rc;
    }
    return 0;
}

int ae_check_idx(vaeb_ae* a, const int32_t* idx, int32_t n) {
    if (!a->data) return fail(VAEB_ERR_STATE, "vaeb_ae_set_data has not been called");
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= a->nrows)
            return fail(VAEB_ERR_ARG, "row index %d out of range [0, %lld)", idx[i], (long long)a->nrows);
    return 0;
}

int ae_reserve(vaeb_ae* a, int n_idx, int n_out) {
    if (n_idx > a->idx_cap) {
        if (a->idx) hipFree(a->idx);
        a->idx = nullptr;
        if (int rc = dalloc(&a->idx, (size_t)n_idx)) return rc;
        a->idx_cap = n_idx;
    }
    if (n_out > a->outs_cap) {
        if (a->outs) hipFree(a->outs);
        a->outs = nullptr;
        if (int rc = dalloc(&a->outs, (size_t)n_out)) return rc;
        a->outs_cap = n_out;
    }
    return 0;
}

// reconstruct / encode / decode over host rows in max_batch chunks.
int ae_predict(vaeb_ae* a, const float* x, int64_t n, float* out, int what) {
    if (!a || !x || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    const vaeb_ae_config& g = a->c;
    const int win = (what == 2) ? g.Dz : g.Dobs;
    const int wout = (what == 1) ? g.Dz : g.Dobs;
    for (int64_t r0 = 0; r0 < n; r0 += g.max_batch) {
        const int rows = (int)std::min<int64_t>(g.max_batch, n - r0);
        HIP_TRY(hipMemcpyAsync(a->xin, x + r0 * win, sizeof(float) * (size_t)rows * win, hipMemcpyHostToDevice, a->s));
        int rc = 0;
        if (what == 2) rc = ae_forward(a, nullptr, 0, nullptr, rows, false, false, a->xin);
        else rc = ae_forward(a, a->xin, rows, nullptr, rows, false, what == 1, nullptr);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(out + r0 * wout, what == 1 ? a->Z : a->Xpr, sizeof(float) * (size_t)rows * wout,
                               hipMemcpyDeviceToHost, a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
    }
    return 0;
}

int ae_xfer(vaeb_ae* a, float* dev, const float* hin, float* hout, int64_t n) {
    if (!a || (!hin && !hout)) return fail(VAEB_ERR_ARG, "null argument");
    if (n != a->P) return fail(VAEB_ERR_ARG, "size mismatch: got %lld, expected %lld", (long long)n, (long long)a->P);
    HIP_TRY(hipStreamSynchronize(a->s));
    if (hin) HIP_TRY(hipMemcpy(dev, hin, sizeof(float) * n, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemcpy(hout, dev, sizeof(float) * n, hipMemcpyDeviceToHost));
    return 0;
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
    auto* a = new vaeb_ae();
    a->c = g;
    if (hipSetDevice(g.device) != hipSuccess || hipStreamCreateWithFlags(&a->s, hipStreamNonBlocking) != hipSuccess) {
        delete a;
        return fail(VAEB_ERR_HIP, "device / stream init failed");
    }
    a->de.push_back(g.Dobs);
    for (int i = 0; i < g.n_enc; ++i) a->de.push_back(g.Denc[i]);
    a->dd.push_back(g.Dz);
    for (int i = 0; i < g.n_dec; ++i) a->dd.push_back(g.Ddec[i]);
    // theta order (ae.py:51,56,64,72)
    int64_t o = 0;
    for (int i = 0; i < g.n_enc; ++i) { a->oWe.push_back(o); o += (int64_t)a->de[i] * a->de[i + 1]; }
    for (int i = 0; i < g.n_enc; ++i) { a->obe.push_back(o); o += a->de[i + 1]; }
    const int64_t HZ = (int64_t)a->de[g.n_enc] * g.Dz;
    if (g.latent == VAEB_AE_LATENT_GAUSS) {   // as the cont output: Wzmu, Wzlv, bzmu, bzlv
        a->oWz = o; o += HZ;
        a->oWzl = o; o += HZ;
        a->obz = o; o += g.Dz;
        a->obzl = o; o += g.Dz;
    } else {
        a->oWz = o; o += HZ;
        a->obz = o; o += g.Dz;
    }
    for (int i = 0; i < g.n_dec; ++i) { a->oWd.push_back(o); o += (int64_t)a->dd[i] * a->dd[i + 1]; }
    for (int i = 0; i < g.n_dec; ++i) { a->obd.push_back(o); o += a->dd[i + 1]; }
    const int64_t HD = (int64_t)a->dd[g.n_dec] * g.Dobs;
    if (g.otype != VAEB_AE_CONT) {   // binary and se: Wout, bout
        a->oWo = o; o += HD;
        a->obo = o; o += g.Dobs;
    } else {
        a->oWo = o; o += HD;        // Wmu
        a->oWl = o; o += HD;        // Wlogs2
        a->obo = o; o += g.Dobs;    // bmu
        a->obl = o; o += g.Dobs;    // blogs2
    }
    a->P = o;
    const int64_t B = g.max_batch;
    int rc = 0;
    rc = rc ? rc : ae_alloc(&a->theta, a->P);
    rc = rc ? rc : ae_alloc(&a->acc, a->P);
    a->H.assign(g.n_enc + 1, nullptr);
    a->dH.assign(g.n_enc + 1, nullptr);
    a->G.assign(g.n_dec + 1, nullptr);
    a->dG.assign(g.n_dec + 1, nullptr);
    for (int i = 1; i <= g.n_enc; ++i) {
        rc = rc ? rc : ae_alloc(&a->H[i], B * a->de[i]);
        rc = rc ? rc : ae_alloc(&a->dH[i], B * a->de[i]);
    }
    for (int i = 1; i <= g.n_dec; ++i) {
        rc = rc ? rc : ae_alloc(&a->G[i], B * a->dd[i]);
        rc = rc ? rc : ae_alloc(&a->dG[i], B * a->dd[i]);
    }
    rc = rc ? rc : ae_alloc(&a->Z, B * g.Dz);
    rc = rc ? rc : ae_alloc(&a->dZ, B * g.Dz);
    rc = rc ? rc : ae_alloc(&a->Xpr, B * g.Dobs);
    rc = rc ? rc : ae_alloc(&a->ls2, B * g.Dobs);
    rc = rc ? rc : ae_alloc(&a->dA, B * g.Dobs);
    rc = rc ? rc : ae_alloc(&a->dA2, B * g.Dobs);
    rc = rc ? rc : ae_alloc(&a->ll, B * cdiv(g.Dobs, 16));
    rc = rc ? rc : ae_alloc(&a->xin, B * std::max(g.Dobs, g.Dz));
    if (ae_gauss(a)) {
        rc = rc ? rc : ae_alloc(&a->mu, B * g.Dz);
        rc = rc ? rc : ae_alloc(&a->lv, B * g.Dz);
        rc = rc ? rc : ae_alloc(&a->dmu, B * g.Dz);
        rc = rc ? rc : ae_alloc(&a->dlv, B * g.Dz);
        rc = rc ? rc : ae_alloc(&a->kl, B * cdiv(g.Dz, 16));
        rc = rc ? rc : dalloc(&a->esum, 1);
    }
    if (ae_iw(a)) {
        rc = rc ? rc : ae_iw_scratch(a);
        rc = rc ? rc : ae_alloc(&a->iw_wt, B);
        rc = rc ? rc : ae_alloc(&a->iw_val, B);
        rc = rc ? rc : dalloc(&a->iw_lw, (size_t)B);
    }
    rc = rc ? rc : ae_reserve(a, (int)B, 1);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(VAEB_ERR_HIP, "device init failed");
    if (rc) { vaeb_ae_destroy(a); return rc; }
    *out = a;
    return 0;
}

int vaeb_ae_destroy(vaeb_ae* a) {
    if (!a) return 0;
    if (a->s) hipStreamSynchronize(a->s);
    std::vector<float*> ps = {a->theta, a->acc, a->data, a->Z, a->dZ, a->Xpr, a->ls2, a->dA, a->dA2, a->ll, a->outs,
                              a->xin, a->mu, a->lv, a->dmu, a->dlv, a->kl, a->eps_in, a->iw, a->iw_wt, a->iw_val,
                              a->sq_rows};
    for (auto* v : {&a->H, &a->G, &a->dH, &a->dG}) ps.insert(ps.end(), v->begin(), v->end());
    for (float* p : ps) if (p) hipFree(p);
    if (a->idx) hipFree(a->idx);
    if (a->iw_yrow) hipFree(a->iw_yrow);
    if (a->esum) hipFree(a->esum);
    if (a->iw_lw) hipFree(a->iw_lw);
    if (a->s) hipStreamDestroy(a->s);
    delete a;
    return 0;
}

int vaeb_ae_num_params(const vaeb_ae* a, int64_t* n) {
    if (!a || !n) return fail(VAEB_ERR_ARG, "null argument");
    *n = a->P;
    return 0;
}

int vaeb_ae_set_data(vaeb_ae* a, const float* x, int64_t n_rows) {
    if (!a || !x || n_rows <= 0) return fail(VAEB_ERR_ARG, "bad data arguments");
    HIP_TRY(hipStreamSynchronize(a->s));
    if (a->data) { hipFree(a->data); a->data = nullptr; }
    if (int rc = dalloc(&a->data, (size_t)n_rows * a->c.Dobs)) return rc;
    HIP_TRY(hipMemcpy(a->data, x, sizeof(float) * (size_t)n_rows * a->c.Dobs, hipMemcpyHostToDevice));
    a->nrows = n_rows;
    return 0;
}

int vaeb_ae_set_params(vaeb_ae* a, const float* f, int64_t n) { return ae_xfer(a, a ? a->theta : nullptr, f, nullptr, n); }
int vaeb_ae_get_params(vaeb_ae* a, float* f, int64_t n) { return ae_xfer(a, a ? a->theta : nullptr, nullptr, f, n); }
int vaeb_ae_set_adagrad_state(vaeb_ae* a, const float* f, int64_t n) { return ae_xfer(a, a ? a->acc : nullptr, f, nullptr, n); }
int vaeb_ae_get_adagrad_state(vaeb_ae* a, float* f, int64_t n) { return ae_xfer(a, a ? a->acc : nullptr, nullptr, f, n); }

int vaeb_ae_train_many(vaeb_ae* a, const int32_t* idx, int32_t n, int32_t batch, float* out) {
    if (!a || !idx || !out || n <= 0 || batch <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (batch > a->c.max_batch) return fail(VAEB_ERR_ARG, "batch %d > max_batch %d", batch, a->c.max_batch);
    if (int rc = ae_check_idx(a, idx, n)) return rc;
    const bool gauss = ae_gauss(a), iw = ae_iw(a);
    if (iw && (int64_t)a->c.iw_samples * std::min(batch, n) > a->c.max_batch)
        return fail(VAEB_ERR_ARG, "iw_samples %d x batch %d > max_batch %d (the stacked sample planes)",
                    a->c.iw_samples, std::min(batch, n), a->c.max_batch);
    if (gauss)
        if (int rc = ae_host_eps_ready(a, iw ? (int64_t)a->c.iw_samples * n : (int64_t)n)) return rc;
    const int nb = cdiv(n, batch);
    if (int rc = ae_reserve(a, n, nb)) return rc;
    HIP_TRY(hipMemcpyAsync(a->idx, idx, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, a->s));
    for (int j = 0; j < nb; ++j) {
        const int lb = j * batch, m = std::min(batch, n - lb);
        if (iw) {
            if (int rc = ae_step_iw(a, a->idx + lb, m, j, lb, n, a->step)) return rc;
            ++a->step;
        } else if (gauss) {   // each step draws at the counter, then advances it
            if (int rc = ae_step(a, a->idx + lb, m, j, ae_noise(a, a->idx + lb, lb, a->step, false))) return rc;
            ++a->step;
        } else if (int rc = ae_step(a, a->idx + lb, m, j)) return rc;
    }
    HIP_TRY(hipMemcpyAsync(out, a->outs, sizeof(float) * (size_t)nb, hipMemcpyDeviceToHost, a->s));
    HIP_TRY(hipStreamSynchronize(a->s));
    return 0;
}

int vaeb_ae_train(vaeb_ae* a, const int32_t* idx, int32_t n, float* out) {
    if (!a || !idx || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    return vaeb_ae_train_many(a, idx, n, n, out);
}

int vaeb_ae_reconstruct(vaeb_ae* a, const float* x, int64_t n, float* out) { return ae_predict(a, x, n, out, 0); }
int vaeb_ae_encode(vaeb_ae* a, const float* x, int64_t n, float* z) { return ae_predict(a, x, n, z, 1); }
int vaeb_ae_decode(vaeb_ae* a, const float* z, int64_t n, float* out) { return ae_predict(a, z, n, out, 2); }

int vaeb_ae_sq_error(vaeb_ae* a, const float* x, int64_t n, double* out_sum, float* out_rows) {
    if (!a || !x || !out_sum || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    const vaeb_ae_config& g = a->c;
    const int nct = cdiv(g.Dobs, 16);
    if (!a->sq_rows)
        if (int rc = ae_alloc(&a->sq_rows, g.max_batch)) return rc;
    if (!a->esum)
        if (int rc = dalloc(&a->esum, 1)) return rc;
    double total = 0.0;
    for (int64_t r0 = 0; r0 < n; r0 += g.max_batch) {
        const int rows = (int)std::min<int64_t>(g.max_batch, n - r0);
        HIP_TRY(hipMemcpyAsync(a->xin, x + r0 * g.Dobs, sizeof(float) * (size_t)rows * g.Dobs, hipMemcpyHostToDevice,
                               a->s));
        // the deterministic forward (Gaussian latent: z = mu), then the mean head's (Y - P)^2 partials
        if (int rc = ae_forward(a, a->xin, rows, nullptr, rows, true, false, nullptr, AeNoise{}, true, true)) return rc;
        hipLaunchKernelGGL(ae::ae_row_sum_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, a->s, a->ll, rows, nct,
                           a->sq_rows);
        CHECK_LAUNCH();
        HIP_TRY(hipMemsetAsync(a->esum, 0, sizeof(double), a->s));
        hipLaunchKernelGGL(iw_sum_kernel, dim3(1), dim3(256), 0, a->s, a->sq_rows, (int64_t)rows, a->esum);
        CHECK_LAUNCH();
        double part = 0.0;
        HIP_TRY(hipMemcpyAsync(&part, a->esum, sizeof(double), hipMemcpyDeviceToHost, a->s));
        if (out_rows)
            HIP_TRY(hipMemcpyAsync(out_rows + r0, a->sq_rows, sizeof(float) * (size_t)rows, hipMemcpyDeviceToHost, a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
        total += part;
    }
    *out_sum = total;
    return 0;
}

// ------------------------------------------------------------------ Gaussian latent
#define AE_NEED_GAUSS(a, fn)                                                                            \
    do {                                                                                                \
        if (!(a)) return fail(VAEB_ERR_ARG, "null argument");                                           \
        if (!ae_gauss(a)) return fail(VAEB_ERR_ARG, fn " needs a VAEB_AE_LATENT_GAUSS context");        \
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
    if (n > a->eps_cap) {
        if (a->eps_in) hipFree(a->eps_in);
        a->eps_in = nullptr;
        a->eps_cap = a->eps_rows = 0;
        if (int rc = dalloc(&a->eps_in, (size_t)n)) return rc;
        a->eps_cap = n;
    }
    HIP_TRY(hipMemcpy(a->eps_in, eps, sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
    a->eps_rows = rows;
    return 0;
}

int vaeb_ae_set_step(vaeb_ae* a, int64_t step) {
    AE_NEED_GAUSS(a, "vaeb_ae_set_step");
    a->step = step;
    return 0;
}

int vaeb_ae_get_step(vaeb_ae* a, int64_t* step) {
    AE_NEED_GAUSS(a, "vaeb_ae_get_step");
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
    for (int64_t r0 = 0; r0 < n; r0 += g.max_batch) {
        const int rows = (int)std::min<int64_t>(g.max_batch, n - r0);
        HIP_TRY(hipMemcpyAsync(a->xin, x + r0 * g.Dobs, sizeof(float) * (size_t)rows * g.Dobs, hipMemcpyHostToDevice,
                               a->s));
        const AeNoise nz = out_z ? ae_noise(a, nullptr, r0, a->step, true) : AeNoise{};
        if (int rc = ae_forward(a, a->xin, rows, nullptr, rows, false, true, nullptr, nz)) return rc;
        const size_t nb = sizeof(float) * (size_t)rows * g.Dz;
        if (out_mu) HIP_TRY(hipMemcpyAsync(out_mu + r0 * g.Dz, a->mu, nb, hipMemcpyDeviceToHost, a->s));
        if (out_lv) HIP_TRY(hipMemcpyAsync(out_lv + r0 * g.Dz, a->lv, nb, hipMemcpyDeviceToHost, a->s));
        if (out_z) HIP_TRY(hipMemcpyAsync(out_z + r0 * g.Dz, a->Z, nb, hipMemcpyDeviceToHost, a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
    }
    return 0;
}

int vaeb_ae_elbo(vaeb_ae* a, const float* x, int64_t n, double* out_sum) {
    AE_NEED_GAUSS(a, "vaeb_ae_elbo");
    if (!x || !out_sum || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    const vaeb_ae_config& g = a->c;
    if (int rc = ae_host_eps_ready(a, n)) return rc;
    double total = 0.0;
    for (int64_t r0 = 0; r0 < n; r0 += g.max_batch) {
        const int rows = (int)std::min<int64_t>(g.max_batch, n - r0);
        HIP_TRY(hipMemcpyAsync(a->xin, x + r0 * g.Dobs, sizeof(float) * (size_t)rows * g.Dobs, hipMemcpyHostToDevice,
                               a->s));
        if (int rc = ae_forward(a, a->xin, rows, nullptr, rows, true, false, nullptr,
                                ae_noise(a, nullptr, r0, a->step, true))) return rc;
        hipLaunchKernelGGL(ae::ae_elbo_kernel, dim3(1), dim3(256), 0, a->s, a->ll, (int64_t)rows * cdiv(g.Dobs, 16),
                           a->kl, (int64_t)rows * cdiv(g.Dz, 16), rows, (float*)nullptr, 0, a->esum);
        CHECK_LAUNCH();
        double part = 0.0;
        HIP_TRY(hipMemcpyAsync(&part, a->esum, sizeof(double), hipMemcpyDeviceToHost, a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
        total += part;
    }
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
    const int B = g.max_batch, nct = cdiv(g.Dobs, 16);
    if (int rc = ae_iw_scratch(a)) return rc;
    IwArgs w{};
    w.nctD = nct; w.K = K; w.logK = (float)std::log((double)K);
    w.lat = a->iw; w.ms = a->iw + B; w.rows = a->iw + 3 * (int64_t)B; w.lp_part = a->ll;
    ae::AeIwArgs q{};
    q.Dz = g.Dz; q.n = n;
    q.eps_mode = a->eps_mode == VAEB_EPS_HOST ? 1 : 0;
    q.seed = a->seed; q.step = a->step; q.eps_in = a->eps_in;
    q.mu = a->mu; q.lv = a->lv; q.z = a->Z; q.lat = a->iw; q.yrow = a->iw_yrow;
    double total = 0.0;
    for (int64_t r0 = 0; r0 < n; r0 += B) {
        const int R = (int)std::min<int64_t>(B, n - r0);
        HIP_TRY(hipMemcpyAsync(a->xin, x + r0 * g.Dobs, sizeof(float) * (size_t)R * g.Dobs, hipMemcpyHostToDevice, a->s));
        if (int rc = ae_forward(a, a->xin, R, nullptr, R, false, true, nullptr)) return rc;   // mu, lv: once
        const int smax = std::max(1, B / R);   // sample planes per pass: S * R <= max_batch stacked rows
        w.Mb = w.Mbp = q.R = R;
        q.row0 = r0;
        for (int k0 = 0; k0 < K; k0 += smax) {
            const int S = std::min(smax, K - k0);
            w.k0 = q.k0 = k0; w.S = q.S = S;
            hipLaunchKernelGGL(ae::ae_iw_sample_kernel, dim3(cdiv(S * R, 16)), dim3(256), 0, a->s, q);
            CHECK_LAUNCH();
            if (int rc = ae_forward(a, a->xin, R, a->iw_yrow, S * R, true, false, a->Z, AeNoise{}, true)) return rc;
            hipLaunchKernelGGL(iw_lse_kernel, dim3(cdiv(R, 256)), dim3(256), 0, a->s, w);
            CHECK_LAUNCH();
        }
        HIP_TRY(hipMemsetAsync(a->esum, 0, sizeof(double), a->s));
        hipLaunchKernelGGL(iw_sum_kernel, dim3(1), dim3(256), 0, a->s, w.rows, (int64_t)R, a->esum);
        CHECK_LAUNCH();
        double part = 0.0;
        HIP_TRY(hipMemcpyAsync(&part, a->esum, sizeof(double), hipMemcpyDeviceToHost, a->s));
        if (out_rows)
            HIP_TRY(hipMemcpyAsync(out_rows + r0, w.rows, sizeof(float) * (size_t)R, hipMemcpyDeviceToHost, a->s));
        HIP_TRY(hipStreamSynchronize(a->s));
        total += part;
    }
    *out_sum = total;
    return 0;
}
#undef AE_NEED_GAUSS

}  // extern "C"
