// engine_clf.inc -- the softmax MLP classifier (include/vaeb_hip.h vaeb_clf_*) on the layer-stack
// kernels (ae_mlp.hpp) and clf_softmax.hpp.  Included by vaeb_hip.hip after engine_ae.inc, whose
// AeLayer, AeRows, AeOptView / ae_put_rule and the optimiser / arena calls' bodies (ae_set_optimizer,
// ae_opt_state, ae_set_opt_step, ae_xfer) it shares.  Each call and
// the helper sequence it runs:
//   vaeb_clf_train(_many)  per batch clf_step: (dropout: clf_mask, training domain) | clf_forward |
//                          clf_softmax (value + P + deltas) | ae_loglik_kernel (the sum) | per layer,
//                          top down, clf_bwd_layer: the data gradient with the old weights, then
//                          that layer's weight gradient + update
//   vaeb_clf_predict       clf_chunks: clf_probs = per draw (clf_mask, evaluation domain) |
//                          clf_forward | clf_softmax (predictions; draws >= 1: the running mean)
//   vaeb_clf_loglik        clf_chunks: clf_forward | clf_softmax (value) | iw_sum_kernel
//   vaeb_clf_accuracy      clf_chunks: clf_probs | clf_hit_kernel | clf_count_kernel
//   vaeb_clf_draw_mask     clf_mask (mask bytes only)
// A dropout context's forward and data-backward launches read the masked arena thm where a MAP
// context's read theta: a pointer, no other kernel.  Its weight-gradient launch is the MASK
// instantiation PAeWgradT<RULE, true>, which updates the real theta.

struct vaeb_clf {
    vaeb_clf_config c{};
    hipStream_t s = nullptr;
    int64_t P = 0;
    AeLayer hid[VAEB_AE_MAX_LAYERS] = {}, out{};   // Din -> Dh..., then Dh[n - 1] -> Dout
    DevOwner mem;                                  // every device allocation; released by vaeb_clf_destroy
    float *theta = nullptr, *acc = nullptr, *acc2 = nullptr;
    float* thm = nullptr;                          // dropout: theta * m of the last draw
    uint8_t* mask = nullptr;                       // dropout: m of the last draw [P]
    float *x = nullptr, *y = nullptr;              // resident Xtr, Ytr
    int64_t nrows = 0;
    int* idx = nullptr;
    int64_t idx_cap = 0;
    float* outs = nullptr;
    int64_t outs_cap = 0;
    float *H[VAEB_AE_MAX_LAYERS + 1] = {}, *dH[VAEB_AE_MAX_LAYERS + 1] = {};   // H[0], dH[0] unused
    float *A = nullptr, *Pr = nullptr, *dA = nullptr, *rowval = nullptr;       // logits, P, deltas, row values
    float *Pacc = nullptr, *xin = nullptr, *yin = nullptr;                     // MC mean; a chunk's host rows
    int* hit = nullptr;
    long long* count = nullptr;
    double* esum = nullptr;
    vaeb_ae_optimizer opt{};
    int64_t opt_t = 0;
    uint64_t seed = 0;
    int64_t step = 0;                              // Philox step counter of the dropout draws
    uint64_t T = 0;                                // keep iff word < T: floor(keep * 2^32)
};

namespace {

bool clf_dropout(const vaeb_clf* c) { return c->c.dropout != 0; }

// m of (step, domain) into mask and theta * m into thm (either may be nullptr).
int clf_mask(vaeb_clf* c, int64_t step, uint32_t domain, float* thm, uint8_t* mask) {
    clf::MaskArgs q{};
    q.theta = c->theta; q.thm = thm; q.mask = mask; q.P = c->P;
    q.seed = c->seed; q.step = step; q.domain = domain; q.T = c->T;
    hipLaunchKernelGGL(clf::clf_mask_kernel, dim3(cdiv(cdiv(c->P, 4), 256)), dim3(256), 0, c->s, q);
    CHECK_LAUNCH();
    return 0;
}

// The arena the network reads for evaluation draw `draw` (-1: theta itself).
int clf_eval_weights(vaeb_clf* c, int draw, const float** th) {
    *th = c->theta;
    if (draw < 0) return 0;
    *th = c->thm;
    return clf_mask(c, c->step, 1u | ((uint32_t)(draw + 1) << 1), c->thm, nullptr);
}

// Hidden activations H[1..n] and the logits A of the M rows of x under the arena th.
int clf_forward(vaeb_clf* c, const float* th, const AeRows& x, int M) {
    const int nh = c->c.n_hidden;
    for (int i = 0; i <= nh; ++i) {
        const AeLayer& l = i < nh ? c->hid[i] : c->out;
        const AeRows in = i == 0 ? x : AeRows{c->H[i], M, nullptr};
        ae::PAeFwd p{};
        p.M = M; p.N = l.N; p.K = l.K;
        p.in = in.p; p.ldin = l.K; p.in_rows = in.rows; p.idx = in.idx;
        p.W = th + l.oW; p.b = th + l.ob;
        p.mode = i < nh ? ae::F_ACT : ae::F_LINEAR; p.act = c->c.act;
        p.out = i < nh ? c->H[i + 1] : c->A;
        launch_bigk<1>(c->s, p);
        CHECK_LAUNCH();
    }
    return 0;
}

// The softmax output on the logits of M rows.  y.p == nullptr: predictions only.
int clf_softmax(vaeb_clf* c, int M, const AeRows& y, float* P, float* d, float* Pacc = nullptr, int l = 0, int L = 1) {
    clf::SoftmaxArgs q{};
    q.a = c->A; q.M = M; q.D = c->c.Dout;
    q.Y = y.p; q.yidx = y.idx; q.loss = c->c.loss;
    q.P = P; q.d = d; q.rowval = c->rowval;
    q.Pacc = Pacc; q.first = l == 0; q.last = l == L - 1; q.invL = (float)(1.0 / L);
    hipLaunchKernelGGL(clf::clf_softmax_kernel, dim3(cdiv(M, 4)), dim3(256), 0, c->s, q);
    CHECK_LAUNCH();
    return 0;
}

// One weight-gradient + update launch for layer l (ae_wgrad's arguments; inv_s2 = 0 without a
// prior), in the MASK instantiation on a dropout context.
int clf_wgrad(vaeb_clf* c, const AeLayer& l, const AeRows& in, const float* dout, int M) {
    auto launch = [&](auto p) {
        p.M = l.K + 1; p.N = l.N; p.K = M;
        p.in = in.p; p.ldin = l.K; p.in_rows = in.rows; p.idx = in.idx; p.Kin = l.K;
        p.dout = dout;
        p.theta = c->theta; p.accum = c->acc; p.offW = l.oW; p.offb = l.ob;
        p.eta = c->opt.eta; p.inv_s2 = c->c.prior ? 1.0f / c->c.s2 : 0.f;
        ae_put_rule(AeOptView{c->opt, c->opt_t, c->acc2}, p);
        if constexpr (std::is_base_of_v<ae::AeMaskArgs<true>, decltype(p)>) p.mask = c->mask;
        launch_bigk<1>(c->s, p);
    };
    const bool dr = clf_dropout(c);
    switch (c->opt.rule) {
    case VAEB_AE_RULE_ADAGRAD:
        if (dr) launch(ae::PAeWgradT<ae::RULE_ADAGRAD, true>{}); else launch(ae::PAeWgrad{});
        break;
    case VAEB_AE_RULE_SGA:
        if (dr) launch(ae::PAeWgradT<ae::RULE_SGA, true>{}); else launch(ae::PAeWgradT<ae::RULE_SGA>{});
        break;
    case VAEB_AE_RULE_ADADELTA:
        if (dr) launch(ae::PAeWgradT<ae::RULE_ADADELTA, true>{}); else launch(ae::PAeWgradT<ae::RULE_ADADELTA>{});
        break;
    case VAEB_AE_RULE_ADAM:
        if (dr) launch(ae::PAeWgradT<ae::RULE_ADAM, true>{}); else launch(ae::PAeWgradT<ae::RULE_ADAM>{});
        break;
    default: return fail(VAEB_ERR_STATE, "unknown update rule %d", c->opt.rule);
    }
    CHECK_LAUNCH();
    return 0;
}

// Backward through layer l with the pre-activation delta d of its output over M rows: the data
// gradient (d W^T) * f'(in) under the arena th into din with the OLD weights (din == nullptr: the
// first layer, none), then the layer's update -- the order of ae_bwd_layer.
int clf_bwd_layer(vaeb_clf* c, const float* th, const AeLayer& l, const float* d, const AeRows& in, int M, float* din) {
    if (din) {
        ae::PAeBwd p{};
        p.M = M; p.N = l.K; p.K = l.N;
        p.dout = d; p.K1 = l.N; p.W = th + l.oW;
        p.h = in.p; p.mode = ae::B_DACT; p.act = c->c.act; p.din = din;
        launch_bigk<1>(c->s, p);
        CHECK_LAUNCH();
    }
    return clf_wgrad(c, l, in, d, M);
}

// One step on the M resident rows idx (a device list): the log-likelihood sum -> outs[slot].
int clf_step(vaeb_clf* c, const int* idx, int M, int slot) {
    const int nh = c->c.n_hidden;
    const float* th = c->theta;
    if (clf_dropout(c)) {
        if (int rc = clf_mask(c, c->step, 0u, c->thm, c->mask)) return rc;
        th = c->thm;
    }
    const AeRows x{c->x, (int)c->nrows, idx};
    if (int rc = clf_forward(c, th, x, M)) return rc;
    if (int rc = clf_softmax(c, M, AeRows{c->y, (int)c->nrows, idx}, c->Pr, c->dA)) return rc;
    hipLaunchKernelGGL(ae::ae_loglik_kernel, dim3(1), dim3(256), 0, c->s, c->rowval, (int64_t)M, 1, c->outs, slot);
    CHECK_LAUNCH();
    if (int rc = clf_bwd_layer(c, th, c->out, c->dA, AeRows{c->H[nh], M, nullptr}, M, c->dH[nh])) return rc;
    for (int i = nh - 1; i > 0; --i)
        if (int rc = clf_bwd_layer(c, th, c->hid[i], c->dH[i + 1], AeRows{c->H[i], M, nullptr}, M, c->dH[i])) return rc;
    if (int rc = clf_bwd_layer(c, th, c->hid[0], c->dH[1], x, M, nullptr)) return rc;
    ++c->step;    // on every context: a schedule means the same with and without dropout
    ++c->opt_t;
    return 0;
}

// Walks n host rows of x [n x Din] (and y [n x Dout] when set) in chunks of at most max_batch rows:
// uploads a chunk to xin (yin), then body(r0, rows).
template <class Body>
int clf_chunks(vaeb_clf* c, const float* x, const float* y, int64_t n, Body body) {
    const int64_t B = c->c.max_batch;
    const int Din = c->c.Din, Dout = c->c.Dout;
    for (int64_t r0 = 0; r0 < n; r0 += B) {
        const int rows = (int)std::min<int64_t>(B, n - r0);
        HIP_TRY(hipMemcpyAsync(c->xin, x + r0 * Din, sizeof(float) * (size_t)rows * Din, hipMemcpyHostToDevice, c->s));
        if (y)
            HIP_TRY(hipMemcpyAsync(c->yin, y + r0 * Dout, sizeof(float) * (size_t)rows * Dout, hipMemcpyHostToDevice, c->s));
        if (int rc = body(r0, rows)) return rc;
    }
    return 0;
}

// P of the chunk in xin: theta as it is (draws == 0, into Pr) or the mean over the evaluation
// draws 0..draws-1 (into Pacc).  *P: where it is.
int clf_probs(vaeb_clf* c, int rows, int draws, const float** P) {
    const AeRows x{c->xin, rows, nullptr};
    if (draws == 0) {
        *P = c->Pr;
        if (int rc = clf_forward(c, c->theta, x, rows)) return rc;
        return clf_softmax(c, rows, AeRows{}, c->Pr, nullptr);
    }
    *P = c->Pacc;
    for (int l = 0; l < draws; ++l) {
        const float* th = nullptr;
        if (int rc = clf_eval_weights(c, l, &th)) return rc;
        if (int rc = clf_forward(c, th, x, rows)) return rc;
        if (int rc = clf_softmax(c, rows, AeRows{}, nullptr, nullptr, c->Pacc, l, draws)) return rc;
    }
    return 0;
}

int clf_check_draws(const vaeb_clf* c, int64_t draws) {
    if (draws < 0 || draws > (1 << 20)) return fail(VAEB_ERR_ARG, "draws = %lld: 0 to 2^20", (long long)draws);
    if (draws >= 1 && !clf_dropout(c))
        return fail(VAEB_ERR_ARG, "draws = %lld on a context without dropout (draws = 0 uses theta)", (long long)draws);
    return 0;
}

}  // namespace

extern "C" {

int vaeb_clf_create(const vaeb_clf_config* cfg, vaeb_clf** out) {
    if (!cfg || !out) return fail(VAEB_ERR_ARG, "null argument");
    const vaeb_clf_config& g = *cfg;
    if (g.Din <= 0 || g.max_batch <= 0) return fail(VAEB_ERR_ARG, "Din and max_batch must be > 0");
    if (g.n_hidden < 1 || g.n_hidden > VAEB_AE_MAX_LAYERS)
        return fail(VAEB_ERR_ARG, "n_hidden = %d: 1 to %d hidden layers", g.n_hidden, VAEB_AE_MAX_LAYERS);
    for (int i = 0; i < g.n_hidden; ++i) if (g.Dh[i] <= 0) return fail(VAEB_ERR_ARG, "Dh[%d] <= 0", i);
    if (g.Dout < 2) return fail(VAEB_ERR_ARG, "Dout = %d: a softmax needs at least 2 classes", g.Dout);
    if (g.act < 0 || g.act > 2) return fail(VAEB_ERR_ARG, "bad activation");
    if (g.loss != VAEB_CLF_BERNOULLI && g.loss != VAEB_CLF_CATEGORICAL)
        return fail(VAEB_ERR_ARG, "loss must be VAEB_CLF_BERNOULLI | _CATEGORICAL (got %d)", g.loss);
    if (g.prior != 0 && g.prior != 1) return fail(VAEB_ERR_ARG, "prior must be 0 (none) or 1 (N(0, s2)) (got %d)", g.prior);
    if (g.prior == 1 && (!(g.s2 > 0.f) || !std::isfinite(g.s2))) return fail(VAEB_ERR_ARG, "prior 1 needs a finite s2 > 0");
    if (!(g.eta > 0.f) || !std::isfinite(g.eta)) return fail(VAEB_ERR_ARG, "eta must be finite and > 0");
    if (g.dropout != 0 && g.dropout != 1) return fail(VAEB_ERR_ARG, "dropout must be 0 or 1 (got %d)", g.dropout);
    if (g.dropout == 1 && (!(g.keep > 0.f) || !(g.keep <= 1.f)))   // NaN fails both
        return fail(VAEB_ERR_ARG, "dropout needs keep in (0, 1] (got %g)", (double)g.keep);
    auto* c = new vaeb_clf();
    c->c = g;
    c->opt = vaeb_ae_optimizer{VAEB_AE_RULE_ADAGRAD, g.eta, 0.f, 0.f, 1e-6f};
    c->T = g.dropout ? (uint64_t)std::floor((double)g.keep * 4294967296.0) : 0;
    for (int i = 0; i < g.n_hidden; ++i) { c->hid[i].K = i ? g.Dh[i - 1] : g.Din; c->hid[i].N = g.Dh[i]; }
    c->out.K = g.Dh[g.n_hidden - 1]; c->out.N = g.Dout;
    // theta order (mlp.py:113): the hidden W's, the hidden b's, Wout, bout
    int64_t o = 0;
    for (int i = 0; i < g.n_hidden; ++i) { c->hid[i].oW = o; o += (int64_t)c->hid[i].K * c->hid[i].N; }
    for (int i = 0; i < g.n_hidden; ++i) { c->hid[i].ob = o; o += c->hid[i].N; }
    c->out.oW = o; o += (int64_t)c->out.K * c->out.N;
    c->out.ob = o; o += c->out.N;
    c->P = o;
    if (c->P >= (1ll << 31)) {   // the tile kernels' 32-bit byte offsets need less anyway
        delete c;
        return fail(VAEB_ERR_ARG, "%lld parameters: the arena holds fewer than 2^31", (long long)o);
    }
    if (hipSetDevice(g.device) != hipSuccess || hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(VAEB_ERR_HIP, "device / stream init failed");
    }
    const int64_t B = g.max_batch;
    int rc = 0;
    rc = rc ? rc : c->mem.alloc(&c->theta, c->P);
    rc = rc ? rc : c->mem.alloc(&c->acc, c->P);
    if (g.dropout) {
        rc = rc ? rc : c->mem.alloc(&c->thm, c->P);
        rc = rc ? rc : c->mem.alloc(&c->mask, c->P);
        rc = rc ? rc : c->mem.alloc(&c->Pacc, B * g.Dout);
    }
    for (int i = 1; i <= g.n_hidden; ++i) {
        rc = rc ? rc : c->mem.alloc(&c->H[i], B * g.Dh[i - 1]);
        rc = rc ? rc : c->mem.alloc(&c->dH[i], B * g.Dh[i - 1]);
    }
    for (float** p : {&c->A, &c->Pr, &c->dA, &c->yin}) rc = rc ? rc : c->mem.alloc(p, B * g.Dout);
    rc = rc ? rc : c->mem.alloc(&c->xin, B * g.Din);
    rc = rc ? rc : c->mem.alloc(&c->rowval, B);
    rc = rc ? rc : c->mem.alloc(&c->hit, B);
    rc = rc ? rc : c->mem.alloc(&c->count, 1);
    rc = rc ? rc : c->mem.alloc(&c->esum, 1);
    rc = rc ? rc : c->mem.grow(&c->idx, &c->idx_cap, B);
    rc = rc ? rc : c->mem.grow(&c->outs, &c->outs_cap, 1);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(VAEB_ERR_HIP, "device init failed");
    if (rc) { vaeb_clf_destroy(c); return rc; }
    *out = c;
    return 0;
}

int vaeb_clf_destroy(vaeb_clf* c) {
    if (!c) return 0;
    if (c->s) hipStreamSynchronize(c->s);
    c->mem.release_all();
    if (c->s) hipStreamDestroy(c->s);
    delete c;
    return 0;
}

int vaeb_clf_num_params(const vaeb_clf* c, int64_t* n) {
    if (!c || !n) return fail(VAEB_ERR_ARG, "null argument");
    *n = c->P;
    return 0;
}

int vaeb_clf_set_data(vaeb_clf* c, const float* x, const float* y, int64_t n_rows) {
    if (!c || !x || !y || n_rows <= 0 || n_rows >= (1ll << 31)) return fail(VAEB_ERR_ARG, "bad data arguments");
    HIP_TRY(hipStreamSynchronize(c->s));
    if (int rc = c->mem.replace(&c->x, n_rows * c->c.Din)) return rc;
    if (int rc = c->mem.replace(&c->y, n_rows * c->c.Dout)) return rc;
    HIP_TRY(hipMemcpy(c->x, x, sizeof(float) * (size_t)n_rows * c->c.Din, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->y, y, sizeof(float) * (size_t)n_rows * c->c.Dout, hipMemcpyHostToDevice));
    c->nrows = n_rows;
    return 0;
}

int vaeb_clf_set_params(vaeb_clf* c, const float* f, int64_t n) { return ae_xfer(c, c ? c->theta : nullptr, f, nullptr, n); }
int vaeb_clf_get_params(vaeb_clf* c, float* f, int64_t n) { return ae_xfer(c, c ? c->theta : nullptr, nullptr, f, n); }

// The update rule and its state: engine_ae.inc's bodies, shared with vaeb_ae.
int vaeb_clf_set_optimizer(vaeb_clf* c, const vaeb_ae_optimizer* o) { return ae_set_optimizer(c, o); }

int vaeb_clf_get_optimizer(vaeb_clf* c, vaeb_ae_optimizer* o) {
    if (!c || !o) return fail(VAEB_ERR_ARG, "null argument");
    *o = c->opt;
    return 0;
}

int vaeb_clf_set_opt_state(vaeb_clf* c, int32_t slot, const float* f, int64_t n) { return ae_opt_state(c, slot, f, nullptr, n); }
int vaeb_clf_get_opt_state(vaeb_clf* c, int32_t slot, float* f, int64_t n) { return ae_opt_state(c, slot, nullptr, f, n); }
int vaeb_clf_set_opt_step(vaeb_clf* c, int64_t t) { return ae_set_opt_step(c, t); }

int vaeb_clf_get_opt_step(vaeb_clf* c, int64_t* t) {
    if (!c || !t) return fail(VAEB_ERR_ARG, "null argument");
    *t = c->opt_t;
    return 0;
}

int vaeb_clf_set_seed(vaeb_clf* c, uint64_t seed) {
    if (!c) return fail(VAEB_ERR_ARG, "null argument");
    c->seed = seed;
    return 0;
}

int vaeb_clf_set_step(vaeb_clf* c, int64_t step) {
    if (!c) return fail(VAEB_ERR_ARG, "null argument");
    if (step < 0) return fail(VAEB_ERR_ARG, "step %lld < 0", (long long)step);
    c->step = step;
    return 0;
}

int vaeb_clf_get_step(vaeb_clf* c, int64_t* step) {
    if (!c || !step) return fail(VAEB_ERR_ARG, "null argument");
    *step = c->step;
    return 0;
}

int vaeb_clf_train_many(vaeb_clf* c, const int32_t* idx, int32_t n, int32_t batch, float* out) {
    if (!c || !idx || !out || n <= 0 || batch <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (batch > c->c.max_batch) return fail(VAEB_ERR_ARG, "batch %d > max_batch %d", batch, c->c.max_batch);
    if (!c->x) return fail(VAEB_ERR_STATE, "vaeb_clf_set_data has not been called");
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= c->nrows)
            return fail(VAEB_ERR_ARG, "row index %d out of range [0, %lld)", idx[i], (long long)c->nrows);
    const int nb = cdiv(n, batch);
    if (int rc = c->mem.grow(&c->idx, &c->idx_cap, n)) return rc;
    if (int rc = c->mem.grow(&c->outs, &c->outs_cap, nb)) return rc;
    HIP_TRY(hipMemcpyAsync(c->idx, idx, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->s));
    for (int j = 0; j < nb; ++j) {
        const int lb = j * batch, m = std::min(batch, n - lb);
        if (int rc = clf_step(c, c->idx + lb, m, j)) return rc;
    }
    HIP_TRY(hipMemcpyAsync(out, c->outs, sizeof(float) * (size_t)nb, hipMemcpyDeviceToHost, c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    return 0;
}

int vaeb_clf_train(vaeb_clf* c, const int32_t* idx, int32_t n, float* out) {
    if (!c || !idx || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (n > c->c.max_batch) return fail(VAEB_ERR_ARG, "n %d > max_batch %d", n, c->c.max_batch);
    return vaeb_clf_train_many(c, idx, n, n, out);
}

int vaeb_clf_predict(vaeb_clf* c, const float* x, int64_t n, int32_t draws, float* out) {
    if (!c || !x || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = clf_check_draws(c, draws)) return rc;
    const int Dout = c->c.Dout;
    return clf_chunks(c, x, nullptr, n, [&](int64_t r0, int rows) {
        const float* P = nullptr;
        if (int rc = clf_probs(c, rows, draws, &P)) return rc;
        HIP_TRY(hipMemcpyAsync(out + r0 * Dout, P, sizeof(float) * (size_t)rows * Dout, hipMemcpyDeviceToHost, c->s));
        HIP_TRY(hipStreamSynchronize(c->s));
        return 0;
    });
}

int vaeb_clf_loglik(vaeb_clf* c, const float* x, const float* y, int64_t n, int32_t draw, double* out_sum) {
    if (!c || !x || !y || !out_sum || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (draw < -1 || draw >= (1 << 20)) return fail(VAEB_ERR_ARG, "draw = %d: -1 (theta) or 0 to 2^20 - 1", draw);
    if (draw >= 0 && !clf_dropout(c)) return fail(VAEB_ERR_ARG, "draw = %d on a context without dropout (-1 uses theta)", draw);
    double total = 0.0;
    const int rc = clf_chunks(c, x, y, n, [&](int64_t, int rows) {
        const float* th = nullptr;
        if (int rc = clf_eval_weights(c, draw, &th)) return rc;
        if (int rc = clf_forward(c, th, AeRows{c->xin, rows, nullptr}, rows)) return rc;
        if (int rc = clf_softmax(c, rows, AeRows{c->yin, rows, nullptr}, nullptr, nullptr)) return rc;
        HIP_TRY(hipMemsetAsync(c->esum, 0, sizeof(double), c->s));
        hipLaunchKernelGGL(iw_sum_kernel, dim3(1), dim3(256), 0, c->s, c->rowval, (int64_t)rows, c->esum);
        CHECK_LAUNCH();
        double part = 0.0;
        HIP_TRY(hipMemcpyAsync(&part, c->esum, sizeof(double), hipMemcpyDeviceToHost, c->s));
        HIP_TRY(hipStreamSynchronize(c->s));
        total += part;
        return 0;
    });
    if (rc) return rc;
    *out_sum = total;
    return 0;
}

int vaeb_clf_accuracy(vaeb_clf* c, const float* x, const float* y, int64_t n, int32_t draws, int64_t* correct) {
    if (!c || !x || !y || !correct || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = clf_check_draws(c, draws)) return rc;
    HIP_TRY(hipMemsetAsync(c->count, 0, sizeof(long long), c->s));
    const int rc = clf_chunks(c, x, y, n, [&](int64_t, int rows) {
        const float* P = nullptr;
        if (int rc = clf_probs(c, rows, draws, &P)) return rc;
        hipLaunchKernelGGL(clf::clf_hit_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, c->s, P, (const float*)c->yin, rows,
                           c->c.Dout, c->hit);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(clf::clf_count_kernel, dim3(1), dim3(256), 0, c->s, (const int*)c->hit, rows, c->count);
        CHECK_LAUNCH();
        HIP_TRY(hipStreamSynchronize(c->s));   // xin / yin are free for the next chunk's upload
        return 0;
    });
    if (rc) return rc;
    long long got = 0;
    HIP_TRY(hipMemcpyAsync(&got, c->count, sizeof(long long), hipMemcpyDeviceToHost, c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    *correct = got;
    return 0;
}

int vaeb_clf_draw_mask(vaeb_clf* c, int64_t step, int32_t draw, uint8_t* out) {
    if (!c || !out) return fail(VAEB_ERR_ARG, "null argument");
    if (!clf_dropout(c)) return fail(VAEB_ERR_ARG, "vaeb_clf_draw_mask needs a dropout context");
    if (step < 0 || draw < -1 || draw >= (1 << 20)) return fail(VAEB_ERR_ARG, "bad step %lld or draw %d", (long long)step, draw);
    if (int rc = clf_mask(c, step, draw < 0 ? 0u : 1u | ((uint32_t)(draw + 1) << 1), nullptr, c->mask)) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->mask, (size_t)c->P, hipMemcpyDeviceToHost, c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    return 0;
}

}  // extern "C"
